// update_plan.hpp -- the arithmetic of lbf_sha1_update_batch: which calls are
// refused, how a call's pieces are spread over launches of bounded size (a
// piece larger than a launch is cut at multiples of 64 bytes), and how one
// launch's bytes are packed into copies.  No HIP, no threads, no environment,
// no I/O, in the way of stage_plan.hpp: every rule here runs in a CPU test
// (tests/c/update_plan_tests.cpp).  update_batch.cpp drives the stream with it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "lbf_hash.h"
#include "stage_plan.hpp"

namespace lbf {

// A chain may absorb this many bytes: its bit count is a 64-bit number
// (iterhash.h:30-31), so the byte count stays below 2^61.
constexpr uint64_t kUpdateMaxTotal = 1ull << 61;

constexpr uint64_t kNoPiece = UINT64_MAX;

inline uint64_t update_state_of(const uint32_t* state_of, uint64_t i) { return state_of ? state_of[i] : i; }

// The checks of one call, all before any GPU work.  Returns the first piece
// that is refused (and why), or kNoPiece.
inline uint64_t update_check(const lbf_sha1_state* states, uint64_t n_states, const uint32_t* state_of,
                             uint64_t base_len, const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                             std::string& why) {
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
    if (st.total > kUpdateMaxTotal || sz > kUpdateMaxTotal - st.total) {
      why = "takes its chain past 2^61 bytes";
      return i;
    }
  }
  if (state_of) {  // two pieces of one state: the order they would be absorbed in is undefined
    std::vector<uint64_t> idx(n);
    for (uint64_t i = 0; i < n; ++i) idx[i] = i;
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

}  // namespace lbf
