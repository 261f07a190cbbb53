// update_seq_plan.hpp -- the arithmetic of lbf_sha1_update_seq_batch and
// lbf_b64_update_seq_batch, the batch calls that take several pieces of one
// state per call: which calls are refused, how a launch's cuts are grouped into
// the chain table the device launches read (sha1_update_seq.hip), and for text
// where a chain's decoded bytes lie on the device and how they come back.
// Cutting a call into launches and packing a launch's bytes into copies stay
// update_plan.hpp's (update_launches cuts in caller order, so a chain's pieces
// may straddle launches, which are ordered); the record invariants and the
// decode bound stay b64_update_plan.hpp's.  No HIP, no threads, no environment,
// no I/O: every rule here runs in a CPU test (tests/c/update_seq_plan_tests.cpp).
// update_seq_batch.cpp drives the stream with it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "b64_update_plan.hpp"
#include "lbf_hash.h"
#include "update_plan.hpp"

namespace lbf {

// The chain table of items whose states are ids[0 .. m): a stable grouping.
// Chains stand in the order their first items stand in `ids`, and a chain's
// items keep their order: order[j] is the item at table position j, chain c's
// items are order[first[c] .. first[c + 1]), and its state is chain_id[c].
// When no state repeats, order is the identity and chain c is item c.
struct ChainTable {
  std::vector<uint32_t> order;     // m entries
  std::vector<uint64_t> chain_id;  // one per chain
  std::vector<uint32_t> first;     // chains + 1 entries
  size_t chains() const { return chain_id.size(); }
};

inline ChainTable chain_table(const std::vector<uint64_t>& ids) {
  ChainTable t;
  const size_t m = ids.size();
  std::unordered_map<uint64_t, uint32_t> chain_of;
  chain_of.reserve(m);
  std::vector<uint32_t> chain(m), count;
  for (size_t k = 0; k < m; ++k) {
    auto it = chain_of.find(ids[k]);
    if (it == chain_of.end()) {
      it = chain_of.emplace(ids[k], (uint32_t)t.chain_id.size()).first;
      t.chain_id.push_back(ids[k]);
      count.push_back(0);
    }
    chain[k] = it->second;
    ++count[it->second];
  }
  t.first.assign(t.chain_id.size() + 1, 0);
  for (size_t c = 0; c < count.size(); ++c) t.first[c + 1] = t.first[c] + count[c];
  std::vector<uint32_t> at(t.first.begin(), t.first.end() - 1);
  t.order.assign(m, 0);
  for (size_t k = 0; k < m; ++k) t.order[at[chain[k]]++] = (uint32_t)k;
  return t;
}

// What the checks keep of a state while they walk the call in piece order.
struct SeqSeen {
  uint64_t first = kNoPiece;  // the state's first piece in the call
  uint64_t final_at = kNoPiece;
  uint64_t sum = 0;  // bytes (characters, for text) of its pieces so far
};

// The checks of one lbf_sha1_update_seq_batch call, all before any GPU work:
// update_check's without "the second piece of one state", the invariants
// against each state as it stands at the call, the 2^61 bound against the SUM
// of the state's pieces, and a final piece that another piece of its state
// follows.  Returns the first piece in caller order at which a fault shows
// (for final-then-more: the final piece, which precedes it), or kNoPiece.
inline uint64_t update_seq_check(const lbf_sha1_state* states, uint64_t n_states, const uint32_t* state_of,
                                 uint64_t base_len, const uint64_t* offsets, const uint32_t* sizes,
                                 const uint8_t* final_flags, uint64_t n, std::string& why) {
  std::unordered_map<uint64_t, SeqSeen> seen;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t o = offsets[i], sz = sizes[i];
    if (o > base_len || sz > base_len - o) {
      why = "lies outside [base, base+base_len)";
      return i;
    }
    const uint64_t s = update_state_of(state_of, i);
    if (s >= n_states) {
      why = "names state " + std::to_string(s) + " of " + std::to_string(n_states);
      return i;
    }
    const lbf_sha1_state& st = states[s];
    if (st.buffered > 63 || st.buffered != st.total % 64) {
      why = "continues a corrupt state (buffered " + std::to_string(st.buffered) + ", total " +
            std::to_string(st.total) + ")";
      return i;
    }
    SeqSeen& q = seen[s];
    if (q.first == kNoPiece) q.first = i;
    if (q.final_at != kNoPiece) {
      why = "is final, but piece " + std::to_string(i) + " of its state " + std::to_string(s) +
            " follows it in the same call";
      return q.final_at;
    }
    // q.sum <= 2^61 - total here, so the subtraction below does not wrap
    if (st.total > kUpdateMaxTotal || q.sum > kUpdateMaxTotal - st.total || sz > kUpdateMaxTotal - st.total - q.sum) {
      why = "takes its chain past 2^61 bytes";
      return i;
    }
    q.sum += sz;
    if (final_flags && final_flags[i]) q.final_at = i;
  }
  return kNoPiece;
}

// The checks of one lbf_b64_update_seq_batch call: b64_update_check's without
// "the second piece of one state", and with pieces of one state that name
// different slots or chunk sizes, a final piece that another piece of its state
// follows, and overlap among the slots of DIFFERENT states only (the device
// clamps `decoded` at 2^61, and the SHA state's total never passes the chunk's
// size, so the sum of a chain's characters needs no bound of its own).
inline uint64_t b64_update_seq_check(const lbf_b64_state* b64, const lbf_sha1_state* sha, uint64_t n_states,
                                     const uint32_t* state_of, uint64_t text_len, const uint64_t* text_offsets,
                                     const uint32_t* text_lens, const uint8_t* final_flags, uint64_t n,
                                     const uint32_t* caps, uint64_t out_len, const uint64_t* out_offsets,
                                     std::string& why) {
  std::unordered_map<uint64_t, SeqSeen> seen;
  std::vector<uint64_t> firsts;  // one piece per state, in caller order
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
    SeqSeen& q = seen[s];
    if (q.first == kNoPiece) {
      q.first = i;
      firsts.push_back(i);
    } else if (out_offsets[q.first] != oo || caps[q.first] != cap) {
      why = "names another slot or chunk size than piece " + std::to_string(q.first) + " of its state " +
            std::to_string(s);
      return i;
    }
    if (q.final_at != kNoPiece) {
      why = "is final, but piece " + std::to_string(i) + " of its state " + std::to_string(s) +
            " follows it in the same call";
      return q.final_at;
    }
    if (final_flags && final_flags[i]) q.final_at = i;
  }
  // slots of different states may touch but not overlap (empty slots hold nothing)
  std::sort(firsts.begin(), firsts.end(), [&](uint64_t a, uint64_t b) {
    return out_offsets[a] != out_offsets[b] ? out_offsets[a] < out_offsets[b] : a < b;
  });
  uint64_t bad = kNoPiece, end = 0;
  for (uint64_t i : firsts) {
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

// Where a launch's chains decode to on the device: one area per chain, in chain
// order.  Chain c has decoded `decoded[c]` bytes with ncarry[c] sextets pending
// into a chunk of cap[c] bytes, and the launch holds chars[c] characters of it
// over all its pieces.  As b64_update_places lays out a piece: the area starts
// at the chain's position mod 64, and its room is the decode bound of the
// chain's characters clipped to what is left of the slot.  Returns the size of
// the launch's area.
inline uint64_t b64_update_seq_places(const std::vector<uint64_t>& decoded, const std::vector<uint32_t>& ncarry,
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

}  // namespace lbf
