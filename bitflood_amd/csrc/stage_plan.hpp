// stage_plan.hpp -- the arithmetic of the host staging pipeline: how a
// descriptor table is ordered, sized, packed into batches, cut into pieces and
// described to the device.  No HIP, no threads, no environment, no I/O: plain
// functions over (file_of, offsets, sizes), so every rule here runs in a CPU
// test (tests/c/stage_plan_tests.cpp).  staging.cpp drives streams with it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <vector>

namespace lbf {

// A descriptor table: chunk k is sizes[k] bytes at offsets[k] of file(k).
struct Table {
  const uint32_t* file_of = nullptr;  // file of each descriptor (null: all in file / buffer 0)
  const uint64_t* offsets = nullptr;
  const uint32_t* sizes = nullptr;
  uint32_t file(uint64_t k) const { return file_of ? file_of[k] : 0; }
};

// The order a worker stages its descriptors in: positions [begin, end) map to
// job indices through `perm` (empty = identity, the common sorted case).
struct Order {
  uint64_t begin = 0;
  std::vector<uint64_t> perm;
  uint64_t operator()(uint64_t pos) const { return perm.empty() ? pos : perm[pos - begin]; }
};

// Source order of descriptors [begin, end): sorted by file, then offset (a
// stable permutation, skipped when the table is already sorted, as every
// file-order table is).
inline Order source_order(const Table& t, uint64_t begin, uint64_t end) {
  Order order;
  order.begin = begin;
  auto before = [&](uint64_t x, uint64_t y) {  // source order: file, then offset
    const uint32_t fx = t.file(x), fy = t.file(y);
    return fx != fy ? fx < fy : t.offsets[x] < t.offsets[y];
  };
  for (uint64_t k = begin + 1; k < end; ++k)
    if (before(k, k - 1)) {
      order.perm.resize(end - begin);
      for (uint64_t q = begin; q < end; ++q) order.perm[q - begin] = q;
      std::stable_sort(order.perm.begin(), order.perm.end(), before);
      break;
    }
  return order;
}

// A run: consecutive descriptors whose byte ranges follow each other in the
// source, staged with one copy.  `dst` is its position in the slot's data
// area (same 16-byte phase as `src`); `avail` is how much of it was read.
struct Run {
  uint64_t src = 0, len = 0, dst = 0, avail = 0;
  uint32_t file = 0;
};

// x rounded up to a multiple of a: the sizes of the areas runs are copied into.
inline uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// Descriptors closer than this to the end of the current run join it: the gap
// is copied along (cheaper than another copy); the 16-byte padding between
// ReadVerifiedChunks' arena slots is the common case.
constexpr uint64_t kJoinGap = 4096;

// A descriptor at offset `o` of `file` joins the run [run_src, run_end) of
// `run_file`: it starts inside the run, or within kJoinGap of its end.
inline bool joins_run(uint32_t run_file, uint64_t run_src, uint64_t run_end, uint32_t file, uint64_t o) {
  return file == run_file && o >= run_src && o <= run_end + kJoinGap;
}

// Bytes that cross the link during one chunk's serial SHA-1 chain: ≈1 µs per
// 64-byte block (conservatively) at ≈50 GB/s of H2D.
inline uint64_t chain_bytes_in_flight(uint64_t largest) {
  return (uint64_t)(50e3 * ((double)largest / 64.0 + 2.0));
}

struct JobSize {
  uint64_t bytes = 0;    // the union of the worker's runs
  uint64_t largest = 0;  // the largest chunk that fits a slot
  uint64_t per = 0;      // the bytes one slot should hold
  uint64_t dev_cap = 0;  // the largest a slot may grow for a long chain
};

// Staging sized to the bytes this worker stages (the union of its runs): a
// quarter of them per slot once they exceed kSplitMin, so a mid-sized job
// still runs as several groups whose copies, H2Ds and kernels overlap; never
// below the largest chunk that fits a slot, and capped at slot_max.
constexpr uint64_t kSplitMin = 32ull << 20;

inline JobSize size_job(const Table& t, const Order& order, uint64_t begin, uint64_t end, uint64_t slot_max,
                        uint64_t dev_budget) {
  JobSize js;
  uint64_t run_src = 0, run_end = 0;
  uint32_t run_file = 0;
  bool open = false;
  for (uint64_t q = begin; q < end; ++q) {
    const uint64_t k = order(q), o = t.offsets[k], sz = t.sizes[k];
    if (sz == 0 || sz + 15 > slot_max) continue;
    js.largest = std::max(js.largest, sz);
    if (open && joins_run(run_file, run_src, run_end, t.file(k), o)) {
      if (o + sz > run_end) js.bytes += o + sz - run_end, run_end = o + sz;
    } else {
      js.bytes += sz;
      run_src = o;
      run_end = o + sz;
      run_file = t.file(k);
      open = true;
    }
  }
  js.per = js.bytes <= kSplitMin ? js.bytes : std::max({kSplitMin, (js.bytes + 3) / 4, js.largest});
  js.per = std::min(js.per, slot_max);
  // Long chains: a batch's kernel lasts one chain (≈1 µs per 64-byte block)
  // and at most ~4 batches are in flight (the hardware queues, see
  // ensure_dev_slots), so batches grow until three of them hold a chain's
  // worth of PCIe time -- beyond LBF_SLOT_MB, within a quarter of the HBM
  // budget and a quarter of the job.
  const uint64_t in_flight = chain_bytes_in_flight(js.largest);
  js.dev_cap = std::max(slot_max, dev_budget / 4);
  if (in_flight > 3 * js.per) js.per = std::max(js.per, std::min({in_flight / 3, js.dev_cap, (js.bytes + 3) / 4}));
  return js;
}

// A group: positions [begin, end) of the order whose bytes fit one slot, packed
// as runs.  run_of gives each position's run, or UINT32_MAX for an empty
// chunk; [0, cursor) of the slot's data area is used.  `oversize`: the chunk
// at `begin` does not fit a slot at all and is the whole group.
struct Group {
  uint64_t begin = 0, end = 0, cursor = 0;
  bool oversize = false;
  std::vector<Run> runs;
  std::vector<uint32_t> run_of;
};

// Pack the group that starts at position i.  A descriptor that starts inside,
// or within kJoinGap of, the current run extends it (a contiguous table is one
// run and one copy; overlapping chunks share their bytes); any other starts a
// new run at the next free position with its 16-byte phase.  So a group holds
// as many chunks as their bytes fit, wherever they lie in the source.  (Round
// 1 grouped by the covering range of consecutive descriptors in caller order,
// which collapsed to one or two chunks per group for a scattered table: 8.5 s
// for 3,000 random chunks of a 160 MiB buffer, tools/staging_probe.py.)
inline void pack_group(const Table& t, const Order& order, uint64_t i, uint64_t end, uint64_t slot_bytes,
                       uint64_t desc_cap, Group& g) {
  g.begin = i;
  g.cursor = 0;
  g.runs.clear();
  g.run_of.clear();
  g.oversize = (uint64_t)t.sizes[order(i)] + 15 > slot_bytes;
  if (g.oversize) {
    g.end = i + 1;
    return;
  }
  uint64_t j = i;
  while (j < end && j - i < desc_cap) {
    const uint64_t k = order(j), o = t.offsets[k], sz = t.sizes[k];
    if (sz == 0) {  // empty chunks take no bytes
      g.run_of.push_back(UINT32_MAX);
      ++j;
      continue;
    }
    if (sz + 15 > slot_bytes) break;  // oversize: the next group starts with it
    Run* r = g.runs.empty() ? nullptr : &g.runs.back();
    if (r && joins_run(r->file, r->src, r->src + r->len, t.file(k), o)) {
      const uint64_t new_len = std::max(r->len, o + sz - r->src);
      if (r->dst + new_len > slot_bytes) break;
      r->len = new_len;
      g.cursor = r->dst + new_len;
    } else {
      const uint64_t p = g.cursor + ((o - g.cursor) & 15u);
      if (p + sz > slot_bytes) break;
      g.runs.push_back(Run{o, sz, p, 0, t.file(k)});
      g.cursor = p + sz;
    }
    g.run_of.push_back((uint32_t)(g.runs.size() - 1));
    ++j;
  }
  g.end = j;
}

// One piece [pstart, pend) of a group's data area on the staged route: the
// parts of the runs inside it, placed relative to pstart.  A run cut by a
// piece boundary is read in parts; once a part comes back short (EOF), the
// rest of that run is unavailable and later pieces skip it.
struct PieceCutter {
  std::vector<bool> cut_short;  // per run: a part of it came back short
  size_t first_run = 0;         // runs before it end at or before the last pstart
  std::vector<Run> parts;
  std::vector<size_t> part_of;  // the run each part belongs to

  explicit PieceCutter(size_t n_runs) : cut_short(n_runs, false) {}

  void cut(const std::vector<Run>& runs, uint64_t pstart, uint64_t pend) {
    parts.clear();
    part_of.clear();
    while (first_run < runs.size() && runs[first_run].dst + runs[first_run].len <= pstart) ++first_run;
    for (size_t r = first_run; r < runs.size() && runs[r].dst < pend; ++r) {
      const uint64_t a0 = std::max(runs[r].dst, pstart), a1 = std::min(runs[r].dst + runs[r].len, pend);
      if (a1 <= a0 || cut_short[r]) continue;
      parts.push_back(Run{runs[r].src + (a0 - runs[r].dst), a1 - a0, a0 - pstart, 0, runs[r].file});
      part_of.push_back(r);
    }
  }
  // after the parts were read: add what each part got to its run
  void fold(std::vector<Run>& runs) {
    for (size_t q = 0; q < parts.size(); ++q) {
      runs[part_of[q]].avail += parts[q].avail;
      if (parts[q].avail < parts[q].len) cut_short[part_of[q]] = true;
    }
  }
};

// What the device is told about one chunk.  An empty chunk of an existing file
// is always readable, wherever it lies: the reference's fseek succeeds past EOF
// and fread of 0 bytes returns 0 (Flood.cpp:259-275); a file that cannot be
// opened leaves every chunk '0' (Flood.cpp:257).  Unreadable chunks must not be
// hashed from stale slot bytes: they get size 0 on the device (result
// discarded).  `r` is the chunk's run, null for an empty chunk.
struct HeaderEntry {
  bool ok;
  uint64_t off;
  uint32_t size;
};
inline HeaderEntry header_entry(const Run* r, bool file_exists, uint64_t o, uint32_t sz) {
  const bool ok = r ? o + sz <= r->src + r->avail : file_exists;
  return HeaderEntry{ok, (r && ok) ? r->dst + (o - r->src) : 0, ok ? sz : 0};
}

// The non-empty chunks cover their span [lo, hi) without a gap, and the span
// is at least min_span bytes.  The union is measured in offset order (a sorted
// copy of the table when it is not sorted already, so repeated chunks count
// once: ADVICE r05).
inline bool gap_free_cover(const uint64_t* offsets, const uint32_t* sizes, uint64_t n, uint64_t min_span,
                           uint64_t& lo, uint64_t& hi) {
  lo = UINT64_MAX, hi = 0;
  uint64_t sum = 0;
  bool sorted = true;
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t o = offsets[k], sz = sizes[k];
    if (sz == 0) continue;
    if (k && o < offsets[k - 1]) sorted = false;
    lo = std::min(lo, o);
    hi = std::max(hi, o + sz);
    sum += sz;
  }
  // the union is at most the sum and at most the span: both must reach the bar
  if (hi <= lo || hi - lo < min_span || sum < hi - lo) return false;
  std::vector<uint64_t> perm;
  if (!sorted) {
    perm.resize(n);
    for (uint64_t k = 0; k < n; ++k) perm[k] = k;
    std::sort(perm.begin(), perm.end(), [&](uint64_t x, uint64_t y) { return offsets[x] < offsets[y]; });
  }
  uint64_t run_end = lo;
  for (uint64_t q = 0; q < n; ++q) {
    const uint64_t k = sorted ? q : perm[q], o = offsets[k], sz = sizes[k];
    if (sz == 0) continue;
    if (o > run_end) return false;  // a gap
    run_end = std::max(run_end, o + sz);
  }
  return true;
}

// Caller slots [off[i], off[i] + len[i]) that the device writes back: sorted,
// checked for overlap (two chunks' results in one byte would race on the
// device), and merged into runs of touching slots.  Each run is one D2H; the
// bytes between runs are the caller's and are never written.  Returns the
// index of a slot that overlaps another, or kNoSlot.
struct SlotRun {
  uint64_t lo, hi;
};
constexpr uint64_t kNoSlot = UINT64_MAX;
inline uint64_t slot_runs(const uint64_t* off, const uint64_t* len, uint64_t n, std::vector<SlotRun>& runs) {
  std::vector<uint64_t> idx;
  idx.reserve(n);
  for (uint64_t i = 0; i < n; ++i)
    if (len[i]) idx.push_back(i);
  std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return off[a] < off[b]; });
  runs.clear();
  for (uint64_t i : idx) {
    if (!runs.empty() && off[i] < runs.back().hi) return i;
    if (!runs.empty() && off[i] == runs.back().hi)
      runs.back().hi += len[i];
    else
      runs.push_back(SlotRun{off[i], off[i] + len[i]});
  }
  return kNoSlot;
}

}  // namespace lbf
