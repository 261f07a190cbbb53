// b64_encode_plan.hpp -- the arithmetic of lbf_b64_encode_update_batch: which
// calls are refused, which characters of its chunk's text a piece writes, where
// a launch's characters lie on the device (at their text position mod 16, so
// the kernel's 16-byte stores apply), and where its tables lie.  Pieces are cut
// into launches by update_plan.hpp's update_launches (an encoder state may be
// stopped at any byte, so its cuts at multiples of 64 do), and the characters
// come back by its copyback_runs.  No HIP, no
// threads, no environment, no I/O: every rule here runs in a CPU test
// (tests/c/b64_encode_plan_tests.cpp).  b64_encode_batch.cpp drives the stream
// with it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
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
  const uint64_t second = second_piece_of_a_state(state_of, n, why);
  if (second != kNoPiece) return second;
  std::vector<uint64_t> all(n);
  for (uint64_t i = 0; i < n; ++i) all[i] = i;
  return slot_overlap(std::move(all), text_offsets, text_caps, why);
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

// Where the tables of one encode launch of m cuts lie in the one block that
// goes up and comes back.
struct EncodeTables {
  uint64_t enc, sha, off, slot, noff, size, cap, nlen, tsize, exp, dig, fin, ver, bytes;
};

inline EncodeTables encode_tables(uint64_t m) {
  TableLayout l;
  EncodeTables t;
  t.enc = l.take(16 * m);
  t.sha = l.take(96 * m);
  t.off = l.take(8 * m);    // piece offsets
  t.slot = l.take(8 * m);   // slot starts
  t.noff = l.take(8 * m);   // new offsets
  t.size = l.take(4 * m);   // piece sizes
  t.cap = l.take(4 * m);
  t.nlen = l.take(4 * m);   // new lengths
  t.tsize = l.take(4 * m);  // text lengths
  t.exp = l.take(20 * m);
  t.dig = l.take(20 * m);
  t.fin = l.take(m);
  t.ver = l.take(m);
  t.bytes = l.bytes;
  return t;
}

}  // namespace lbf
