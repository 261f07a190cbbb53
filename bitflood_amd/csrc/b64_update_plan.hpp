// b64_update_plan.hpp -- the arithmetic of the piecewise text calls,
// lbf_b64_update_batch (one piece per state and call) and
// lbf_b64_update_seq_batch (several, decoded in the caller's order): which calls
// are refused, how many bytes a chain's text can decode to at most, where a
// launch's decoded bytes lie on the device (at their chain position mod 64, so
// the update kernel's aligned loop applies), and where a launch's tables lie.
// Text is cut into launches, packed into copies, grouped into chains and its
// bytes copied back by update_plan.hpp (a base64 state may be stopped at any
// character, so its cuts at multiples of 64 do).  No HIP, no threads, no
// environment, no I/O: every rule here runs in a CPU test
// (tests/c/b64_update_plan_tests.cpp, tests/c/update_seq_plan_tests.cpp).
// update_batch.cpp drives the stream with it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "b64_encode_update.hpp"
#include "lbf_hash.h"
#include "update_plan.hpp"

namespace lbf {

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

// The per-piece rules of the text calls, in the order they are reported: piece
// i (l characters at o of the text, state s, a chunk of cap bytes in the slot at
// oo) against the text, the bound on a chunk, the output, the state arrays and
// the state pair as it stands at the call.  False, with `why`, when one fails.
inline bool b64_piece_ok(const lbf_b64_state* b64, const lbf_sha1_state* sha, uint64_t n_states, uint64_t s,
                         uint64_t text_len, uint64_t o, uint64_t l, uint64_t cap, uint64_t out_len, uint64_t oo,
                         std::string& why) {
  if (o > text_len || l > text_len - o) {
    why = "has text outside [text, text+text_len)";
    return false;
  }
  if (cap > b64e::kEncMaxChunk) {
    why = "is of a chunk of " + std::to_string(cap) + " bytes, more than 1 GiB";
    return false;
  }
  if (oo > out_len || cap > out_len - oo) {
    why = "has its slot outside [out, out+out_len)";
    return false;
  }
  if (s >= n_states) {
    why = "names state " + std::to_string(s) + " of " + std::to_string(n_states);
    return false;
  }
  const std::string fault = b64_state_fault(b64[s], sha[s], cap);
  if (!fault.empty()) {
    why = "continues a corrupt state: " + fault;
    return false;
  }
  return true;
}

// Slots of different states may touch but not overlap (empty slots hold
// nothing).  `pieces` names one piece per state; returns the first of them in
// caller order whose slot begins inside an earlier-starting one, or kNoPiece.
inline uint64_t slot_overlap(std::vector<uint64_t> pieces, const uint64_t* offsets, const uint32_t* caps,
                             std::string& why) {
  std::sort(pieces.begin(), pieces.end(),
            [&](uint64_t a, uint64_t b) { return offsets[a] != offsets[b] ? offsets[a] < offsets[b] : a < b; });
  uint64_t bad = kNoPiece, end = 0;
  for (uint64_t i : pieces) {
    if (caps[i] == 0) continue;
    if (offsets[i] < end) bad = std::min(bad, i);
    end = std::max(end, offsets[i] + caps[i]);
  }
  if (bad != kNoPiece) why = "has a slot that overlaps another state's";
  return bad;
}

// The checks of one lbf_b64_update_batch call, all before any GPU work: the
// per-piece rules over the whole call, "the second piece of one state", then
// overlap among the slots.  Returns the first piece that is refused (and why),
// or kNoPiece.
inline uint64_t b64_update_check(const lbf_b64_state* b64, const lbf_sha1_state* sha, uint64_t n_states,
                                 const uint32_t* state_of, uint64_t text_len, const uint64_t* text_offsets,
                                 const uint32_t* text_lens, uint64_t n, const uint32_t* caps, uint64_t out_len,
                                 const uint64_t* out_offsets, std::string& why) {
  std::vector<uint64_t> all(n);
  for (uint64_t i = 0; i < n; ++i) {
    all[i] = i;
    if (!b64_piece_ok(b64, sha, n_states, update_state_of(state_of, i), text_len, text_offsets[i], text_lens[i],
                      caps[i], out_len, out_offsets[i], why))
      return i;
  }
  const uint64_t second = second_piece_of_a_state(state_of, n, why);
  return second != kNoPiece ? second : slot_overlap(std::move(all), out_offsets, caps, why);
}

// The checks of one lbf_b64_update_seq_batch call: the same per-piece rules,
// walked in caller order; a state may repeat, but its pieces name one slot and
// one chunk size and none follows a final piece of it; then overlap among the
// slots of DIFFERENT states only (the device clamps `decoded` at 2^61, and the
// SHA state's total never passes the chunk's size, so the sum of a chain's
// characters needs no bound of its own).
inline uint64_t b64_update_seq_check(const lbf_b64_state* b64, const lbf_sha1_state* sha, uint64_t n_states,
                                     const uint32_t* state_of, uint64_t text_len, const uint64_t* text_offsets,
                                     const uint32_t* text_lens, const uint8_t* final_flags, uint64_t n,
                                     const uint32_t* caps, uint64_t out_len, const uint64_t* out_offsets,
                                     std::string& why) {
  std::unordered_map<uint64_t, SeqSeen> seen;
  std::vector<uint64_t> firsts;  // one piece per state, in caller order
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t s = update_state_of(state_of, i);
    if (!b64_piece_ok(b64, sha, n_states, s, text_len, text_offsets[i], text_lens[i], caps[i], out_len,
                      out_offsets[i], why))
      return i;
    SeqSeen& q = seen[s];
    if (q.first == kNoPiece) {
      q.first = i;
      firsts.push_back(i);
    } else if (out_offsets[q.first] != out_offsets[i] || caps[q.first] != caps[i]) {
      why = "names another slot or chunk size than piece " + std::to_string(q.first) + " of its state " +
            std::to_string(s);
      return i;
    }
    if (q.final_at != kNoPiece) return follows_final(q, i, s, why);
    if (final_flags && final_flags[i]) q.final_at = i;
  }
  return slot_overlap(std::move(firsts), out_offsets, caps, why);
}

// Where a chain's text decodes to on the device.
struct B64Place {
  uint64_t dev = 0;   // device position of its first new byte, = (chain position) mod 64
  uint64_t room = 0;  // the most the launch can write there
  uint64_t slot = 0;  // the kernel's slot start: dev - chain position, mod 2^64
};

// One area per chain of a launch, in chain order (a chain of the one-piece call
// is one cut).  Chain c has decoded `decoded[c]` bytes with ncarry[c] sextets
// pending into a chunk of cap[c] bytes, and the launch holds chars[c] characters
// of it over all its pieces.  The kernel writes chain positions [min(decoded,
// cap), cap) at most, so the room is the decode bound of the chain's characters
// clipped to what is left of the slot; areas follow one another, each moved up
// to its chain position mod 64.  Returns the size of the launch's area.
inline uint64_t b64_update_places(const std::vector<uint64_t>& decoded, const std::vector<uint32_t>& ncarry,
                                  const std::vector<uint64_t>& chars, const std::vector<uint32_t>& cap,
                                  std::vector<B64Place>& places) {
  places.assign(decoded.size(), B64Place{});
  uint64_t cursor = 0;
  for (size_t c = 0; c < decoded.size(); ++c) {
    const uint64_t at = std::min<uint64_t>(decoded[c], cap[c]);
    B64Place& p = places[c];
    p.room = std::min<uint64_t>(b64_decode_bound(ncarry[c] & 3u, chars[c]), cap[c] - at);
    p.dev = cursor + ((at - cursor) & 63u);
    p.slot = p.dev - at;  // mod 2^64: the kernel adds the chain position back
    cursor = p.dev + p.room;
  }
  return cursor;
}

// Where the tables of one text launch of m cuts in nc chains lie in the one
// block that goes up and comes back: the chains' state pairs, then a table per
// cut in table order; the seq launch has chain_first among them.
struct TextTables {
  uint64_t b64, sha, toff, slot, poff, first, tlen, cap, psize, osize, lines, flat, exp, dig, fin, ver, bytes;
};

inline TextTables text_tables(uint64_t m, uint64_t nc, bool seq) {
  TableLayout l;
  TextTables t;
  t.b64 = l.take(16 * nc);
  t.sha = l.take(96 * nc);
  t.toff = l.take(8 * m);   // text offsets
  t.slot = l.take(8 * m);   // slot starts
  t.poff = l.take(8 * m);   // piece offsets
  t.first = l.take(seq ? 4 * (nc + 1) : 0);
  t.tlen = l.take(4 * m);   // text lengths
  t.cap = l.take(4 * m);    // chunk sizes
  t.psize = l.take(4 * m);  // piece sizes
  t.osize = l.take(4 * m);  // decoded lengths
  t.lines = l.take(4 * m);  // line-path characters
  t.flat = l.take(4 * m);   // flat-path characters
  t.exp = l.take(20 * m);
  t.dig = l.take(20 * m);
  t.fin = l.take(m);
  t.ver = l.take(m);
  t.bytes = l.bytes;
  return t;
}

}  // namespace lbf
