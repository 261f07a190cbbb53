// update_plan.hpp -- the arithmetic of the piecewise hash calls,
// lbf_sha1_update_batch (one piece per state and call) and
// lbf_sha1_update_seq_batch (several, absorbed in the caller's order): which
// calls are refused, how a call's pieces are spread over launches of bounded
// size (a piece larger than a launch is cut at multiples of 64 bytes), how one
// launch's bytes are packed into copies, how a launch's cuts are grouped into
// the chain table the device launches read, and where a launch's tables lie.
// The text and encode calls (b64_update_plan.hpp, b64_encode_plan.hpp) cut,
// pack, group and copy back by the same functions.  No HIP, no threads, no
// environment, no I/O, in the way of stage_plan.hpp: every rule here runs in a
// CPU test (tests/c/update_plan_tests.cpp, tests/c/update_seq_plan_tests.cpp).
// update_batch.cpp drives the stream with it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "lbf_hash.h"
#include "stage_plan.hpp"

namespace lbf {

// A chain may absorb this many bytes: its bit count is a 64-bit number
// (iterhash.h:30-31), so the byte count stays below 2^61.
constexpr uint64_t kUpdateMaxTotal = 1ull << 61;

constexpr uint64_t kNoPiece = UINT64_MAX;

inline uint64_t update_state_of(const uint32_t* state_of, uint64_t i) { return state_of ? state_of[i] : i; }

// What the checks keep of a state while they walk a seq call in piece order.
struct SeqSeen {
  uint64_t first = kNoPiece;  // the state's first piece in the call
  uint64_t final_at = kNoPiece;
  uint64_t sum = 0;  // bytes of its pieces so far
};

// "is final, but piece i of its state follows": the final piece is the one named.
inline uint64_t follows_final(const SeqSeen& q, uint64_t i, uint64_t s, std::string& why) {
  why = "is final, but piece " + std::to_string(i) + " of its state " + std::to_string(s) +
        " follows it in the same call";
  return q.final_at;
}

// The per-piece rules of the hash calls, in the order they are reported: piece i
// ([o, o + sz) of the source, state s) against the source, the state array, the
// state as it stands at the call and the 2^61 bound.  With `seen` (the seq
// call: what the state's earlier pieces left) a final piece before this one is
// a fault, and the bound holds for the sum of the state's pieces.  Returns the
// piece to name (i, or the final piece that i follows), or kNoPiece.
inline uint64_t update_piece_fault(const lbf_sha1_state* states, uint64_t n_states, uint64_t s, uint64_t base_len,
                                   uint64_t o, uint64_t sz, uint64_t i, const SeqSeen* seen, std::string& why) {
  if (o > base_len || sz > base_len - o) {
    why = "lies outside [base, base+base_len)";
    return i;
  }
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
  if (seen && seen->final_at != kNoPiece) return follows_final(*seen, i, s, why);
  const uint64_t sum = seen ? seen->sum : 0;
  // sum <= 2^61 - total where it is read, so the last subtraction does not wrap
  if (st.total > kUpdateMaxTotal || sum > kUpdateMaxTotal - st.total || sz > kUpdateMaxTotal - st.total - sum) {
    why = "takes its chain past 2^61 bytes";
    return i;
  }
  return kNoPiece;
}

// The one-piece calls' rule over the whole call: two pieces of one state have no
// defined order.  Names the first piece in caller order that is a state's second.
inline uint64_t second_piece_of_a_state(const uint32_t* state_of, uint64_t n, std::string& why) {
  if (!state_of) return kNoPiece;
  std::vector<uint64_t> idx(n);
  for (uint64_t i = 0; i < n; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(),
            [&](uint64_t a, uint64_t b) { return state_of[a] != state_of[b] ? state_of[a] < state_of[b] : a < b; });
  uint64_t bad = kNoPiece;
  for (uint64_t k = 1; k < n; ++k)
    if (state_of[idx[k]] == state_of[idx[k - 1]]) bad = std::min(bad, idx[k]);
  if (bad != kNoPiece) why = "is the second piece of state " + std::to_string(state_of[bad]) + " in one call";
  return bad;
}

// The checks of one lbf_sha1_update_batch call, all before any GPU work: the
// per-piece rules over the whole call, then "the second piece of one state".
// Returns the first piece that is refused (and why), or kNoPiece.
inline uint64_t update_check(const lbf_sha1_state* states, uint64_t n_states, const uint32_t* state_of,
                             uint64_t base_len, const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                             std::string& why) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t bad = update_piece_fault(states, n_states, update_state_of(state_of, i), base_len, offsets[i],
                                            sizes[i], i, nullptr, why);
    if (bad != kNoPiece) return bad;
  }
  return second_piece_of_a_state(state_of, n, why);
}

// The checks of one lbf_sha1_update_seq_batch call: the same per-piece rules,
// walked in caller order with what each state's earlier pieces left (the
// invariants hold against the state as it stands at the call, the 2^61 bound
// against the SUM of the state's pieces), so a state may repeat, but no piece
// may follow a final piece of its state.  Returns the first piece in caller
// order at which a fault shows (for final-then-more: the final piece, which
// precedes it), or kNoPiece.
inline uint64_t update_seq_check(const lbf_sha1_state* states, uint64_t n_states, const uint32_t* state_of,
                                 uint64_t base_len, const uint64_t* offsets, const uint32_t* sizes,
                                 const uint8_t* final_flags, uint64_t n, std::string& why) {
  std::unordered_map<uint64_t, SeqSeen> seen;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t s = update_state_of(state_of, i);
    SeqSeen& q = seen[s];
    const uint64_t bad = update_piece_fault(states, n_states, s, base_len, offsets[i], sizes[i], i, &q, why);
    if (bad != kNoPiece) return bad;
    q.sum += sizes[i];
    if (final_flags && final_flags[i]) q.final_at = i;
  }
  return kNoPiece;
}

// A cut: bytes [off, off + size) of the source, part (or all) of piece `piece`.
// `last` marks the piece's last cut, the one that carries its final flag.
struct UpdateCut {
  uint64_t piece = 0, off = 0;
  uint32_t size = 0;
  bool last = false;
};

// Launches of at most `cap` piece bytes each (cap is rounded down to a multiple
// of 64, at least 64), pieces in caller order.  A piece that fits what is left
// of the current launch joins it; one that fits a launch starts the next; a
// piece larger than a launch is cut at multiples of 64 bytes of the piece, one
// cut per launch in order (its cuts never share a launch: they continue one
// state), the first filling what is left of the current launch.  Empty pieces
// take no room.
inline std::vector<std::vector<UpdateCut>> update_launches(const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                                                           uint64_t cap) {
  cap = std::max<uint64_t>(64, cap & ~63ull);
  std::vector<std::vector<UpdateCut>> launches(1);
  uint64_t used = 0;
  auto next_launch = [&] {
    launches.emplace_back();
    used = 0;
  };
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t sz = sizes[i];
    if (sz <= cap) {
      if (sz > cap - used) next_launch();
      launches.back().push_back(UpdateCut{i, offsets[i], (uint32_t)sz, true});
      used += sz;
      continue;
    }
    uint64_t done = 0;
    while (done < sz) {
      uint64_t room = (cap - used) & ~63ull;
      if (room == 0) {
        next_launch();
        room = cap;
      }
      const uint64_t take = std::min(room, sz - done);
      const bool last = done + take == sz;
      launches.back().push_back(UpdateCut{i, offsets[i] + done, (uint32_t)take, last});
      used += take;
      done += take;
      if (!last) next_launch();
    }
  }
  if (launches.back().empty() && launches.size() > 1) launches.pop_back();
  return launches;
}

// One launch's bytes as runs (stage_plan.hpp): a cut that starts inside the
// current run, or exactly at its end, extends it (adjacent pieces travel in
// one copy, and only pieces' bytes are read); any other starts a new run at
// the next free position with the source's 16-byte phase.  dev_off[k] is where
// cut k's bytes start in the launch's data area; returns the area's size.
inline uint64_t update_runs(const std::vector<UpdateCut>& cuts, std::vector<Run>& runs, std::vector<uint64_t>& dev_off) {
  runs.clear();
  dev_off.assign(cuts.size(), 0);
  uint64_t cursor = 0;
  for (size_t k = 0; k < cuts.size(); ++k) {
    const uint64_t o = cuts[k].off, sz = cuts[k].size;
    if (sz == 0) continue;
    Run* r = runs.empty() ? nullptr : &runs.back();
    if (r && o >= r->src && o <= r->src + r->len) {
      r->len = std::max(r->len, o + sz - r->src);
      cursor = r->dst + r->len;
    } else {
      const uint64_t p = cursor + ((o - cursor) & 15u);
      runs.push_back(Run{o, sz, p, sz, 0});
      cursor = p + sz;
      r = &runs.back();
    }
    dev_off[k] = r->dst + (o - r->src);
  }
  return cursor;
}

// Copy-back: cut k put size[k] bytes at device position dev[k], which belong at
// host position host[k].  Ranges that touch on both sides travel as one run
// (stage_plan.hpp's Run: src = device, dst = host).
inline void copyback_runs(const std::vector<uint64_t>& dev, const std::vector<uint64_t>& host,
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

// Below this many bytes per run on average what a launch produced comes back as
// one copy of the launch's area and is scattered on the host, so that thousands
// of small pieces do not cost a copy each.  The figure is a guess, not a
// measured crossover.
constexpr uint64_t kDirectRunBytes = 64 << 10;

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

// chain_table(ids) for ids of which none repeats (a launch of the one-piece
// calls: checked), without the hash map.
inline ChainTable identity_table(const std::vector<uint64_t>& ids) {
  ChainTable t;
  t.chain_id = ids;
  t.order.resize(ids.size());
  t.first.resize(ids.size() + 1);
  for (size_t k = 0; k < ids.size(); ++k) t.order[k] = t.first[k] = (uint32_t)k;
  t.first[ids.size()] = (uint32_t)ids.size();
  return t;
}

// The chain table of one launch's cuts, by the state each cut's piece names.
inline ChainTable table_of(const std::vector<UpdateCut>& cuts, const uint32_t* state_of, bool seq) {
  std::vector<uint64_t> ids(cuts.size());
  for (size_t k = 0; k < cuts.size(); ++k) ids[k] = update_state_of(state_of, cuts[k].piece);
  return seq ? chain_table(ids) : identity_table(ids);
}

// Hands out consecutive offsets of one block of tables, in the order asked.
struct TableLayout {
  uint64_t bytes = 0;
  uint64_t take(uint64_t size) {
    const uint64_t at = bytes;
    bytes += size;
    return at;
  }
};

// Where the tables of one hash launch of m cuts in nc chains lie in the block
// that goes up: the chains' states first (they alone come back), then a table
// per cut in table order; the seq launch has chain_first among them.  Digests
// and verdicts are a block of their own (20 m | m).
struct HashTables {
  uint64_t states, off, first, size, exp, fin, bytes;
};

inline HashTables hash_tables(uint64_t m, uint64_t nc, bool seq) {
  TableLayout l;
  HashTables t;
  t.states = l.take(96 * nc);
  t.off = l.take(8 * m);
  t.first = l.take(seq ? 4 * (nc + 1) : 0);
  t.size = l.take(4 * m);
  t.exp = l.take(20 * m);
  t.fin = l.take(m);
  t.bytes = l.bytes;
  return t;
}

}  // namespace lbf
