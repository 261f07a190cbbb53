// CPU test of the staging planner (bitflood_amd/csrc/stage_plan.hpp).  Links
// nothing of the library: the planner is plain arithmetic on descriptor tables.
// Expected values are written out from the rules, with slots of about 1 KiB and
// 4 descriptors per group so that every edge is a handful of descriptors.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "stage_plan.hpp"

using namespace lbf;

static int g_failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++g_failed;                                                \
    }                                                            \
  } while (0)

struct Tab {
  std::vector<uint32_t> f;
  std::vector<uint64_t> o;
  std::vector<uint32_t> s;
  void add(uint32_t file, uint64_t off, uint32_t size) {
    f.push_back(file);
    o.push_back(off);
    s.push_back(size);
  }
  uint64_t n() const { return o.size(); }
  Table table() const {
    Table t;
    t.file_of = f.data();
    t.offsets = o.data();
    t.sizes = s.data();
    return t;
  }
};

static constexpr uint64_t kSlot = 1024, kCap = 4, kMiB = 1ull << 20;

static Group pack(const Tab& t, uint64_t i, uint64_t slot = kSlot, uint64_t cap = kCap) {
  const Table tb = t.table();
  const Order order = source_order(tb, 0, t.n());
  Group g;
  pack_group(tb, order, i, t.n(), slot, cap, g);
  return g;
}

static void test_runs() {
  {  // a contiguous table is one run, placed at its source's phase
    Tab t;
    t.add(0, 37, 100), t.add(0, 137, 100), t.add(0, 237, 100);
    const Group g = pack(t, 0);
    CHECK(!g.oversize && g.begin == 0 && g.end == 3 && g.cursor == 305);
    CHECK(g.runs.size() == 1 && g.runs[0].src == 37 && g.runs[0].len == 300 && g.runs[0].dst == (37 & 15));
    CHECK(g.run_of == std::vector<uint32_t>({0, 0, 0}));
  }
  {  // a gap of exactly kJoinGap joins, and the run's length includes the gap
    Tab t;
    t.add(0, 0, 100), t.add(0, 100 + kJoinGap, 50);
    const Group g = pack(t, 0, 8192);
    CHECK(g.end == 2 && g.runs.size() == 1 && g.runs[0].len == 100 + kJoinGap + 50 && g.cursor == 100 + kJoinGap + 50);
  }
  {  // one byte more starts a run at the next position with the source's phase
    Tab t;
    t.add(0, 3, 100), t.add(0, 103 + kJoinGap + 1, 50);
    const Group g = pack(t, 0, 8192);
    CHECK(g.end == 2 && g.runs.size() == 2 && g.runs[0].dst == 3);
    const uint64_t cursor_before = 103, o = 103 + kJoinGap + 1;
    CHECK(g.runs[1].src == o && g.runs[1].len == 50 && g.runs[1].dst == 104);
    CHECK(g.runs[1].dst % 16 == o % 16 && g.runs[1].dst >= cursor_before && g.runs[1].dst < cursor_before + 16);
    CHECK(g.cursor == 154 && g.run_of == std::vector<uint32_t>({0, 1}));
  }
  {  // duplicate, contained and overlapping chunks extend the run by max only
    Tab t;
    t.add(0, 10, 100), t.add(0, 10, 100), t.add(0, 20, 30), t.add(0, 60, 100);
    const Group g = pack(t, 0);
    CHECK(g.end == 4 && g.runs.size() == 1 && g.runs[0].src == 10 && g.runs[0].len == 150 && g.runs[0].dst == 10);
    CHECK(g.cursor == 160 && g.run_of == std::vector<uint32_t>({0, 0, 0, 0}));
  }
  {  // adjacent offsets in different files never join
    Tab t;
    t.add(0, 0, 100), t.add(1, 100, 100);
    const Group g = pack(t, 0);
    CHECK(g.end == 2 && g.runs.size() == 2 && g.runs[0].file == 0 && g.runs[1].file == 1);
    CHECK(g.runs[0].len == 100 && g.runs[1].src == 100 && g.runs[1].dst == 100 + ((100 - 100) & 15) && g.cursor == 200);
  }
  {  // an empty chunk takes a descriptor, no bytes, and counts toward desc_cap
    Tab t;
    t.add(0, 5, 0), t.add(0, 6, 0), t.add(0, 7, 0), t.add(0, 8, 0), t.add(0, 9, 100);
    const Group g = pack(t, 0);
    CHECK(g.end == 4 && g.runs.empty() && g.cursor == 0);
    CHECK(g.run_of == std::vector<uint32_t>({UINT32_MAX, UINT32_MAX, UINT32_MAX, UINT32_MAX}));
    const Group g2 = pack(t, 4);
    CHECK(g2.begin == 4 && g2.end == 5 && g2.runs.size() == 1 && g2.runs[0].dst == 9 && g2.cursor == 109);
  }
}

static void test_group_ends() {
  {  // a chunk with sz + 15 > slot_bytes ends the group, and heads the next as oversize
    Tab t;
    t.add(0, 0, 100), t.add(0, 5000, 1010), t.add(0, 7000, 10);
    const Group g = pack(t, 0);
    CHECK(g.end == 1 && !g.oversize && g.cursor == 100);
    const Group over = pack(t, 1);
    CHECK(over.oversize && over.begin == 1 && over.end == 2 && over.runs.empty() && over.run_of.empty());
    Tab fits;  // 1009 + 15 == slot_bytes: the largest chunk that is not oversize
    fits.add(0, 15, 1009);
    const Group f = pack(fits, 0);
    CHECK(!f.oversize && f.end == 1 && f.runs[0].dst == 15 && f.cursor == 1024);
  }
  {  // a run extension past slot_bytes
    Tab t;
    t.add(0, 0, 600), t.add(0, 600, 500);
    const Group g = pack(t, 0);
    CHECK(g.end == 1 && g.runs.size() == 1 && g.runs[0].len == 600 && g.cursor == 600);
    Tab exact;  // to exactly slot_bytes it still fits
    exact.add(0, 0, 600), exact.add(0, 600, 424);
    CHECK(pack(exact, 0).end == 2 && pack(exact, 0).cursor == 1024);
  }
  {  // a new run that does not fit: p = 600 + ((10000 - 600) & 15) = 608, 608 + 500 > 1024
    Tab t;
    t.add(0, 0, 600), t.add(0, 10000, 500);
    const Group g = pack(t, 0);
    CHECK(g.end == 1 && g.runs.size() == 1 && g.cursor == 600);
    Tab fits;
    fits.add(0, 0, 600), fits.add(0, 10000, 416);
    const Group f = pack(fits, 0);
    CHECK(f.end == 2 && f.runs[1].dst == 608 && f.cursor == 1024);
  }
  {  // desc_cap descriptors
    Tab t;
    for (int k = 0; k < 5; ++k) t.add(0, 10 * k, 10);
    const Group g = pack(t, 0);
    CHECK(g.end == 4 && g.runs.size() == 1 && g.runs[0].len == 40);
    CHECK(pack(t, 4).end == 5);
  }
}

static void test_order() {
  Tab t;
  t.add(1, 5, 1), t.add(0, 9, 1), t.add(0, 3, 1), t.add(1, 5, 1), t.add(0, 3, 1);
  const Order all = source_order(t.table(), 0, 5);
  CHECK(all.perm == std::vector<uint64_t>({2, 4, 1, 0, 3}));  // (file, offset), equal keys in table order
  CHECK(all(0) == 2 && all(4) == 3);
  const Order tail = source_order(t.table(), 1, 5);
  CHECK(tail.begin == 1 && tail.perm == std::vector<uint64_t>({2, 4, 1, 3}) && tail(1) == 2 && tail(4) == 3);
  Tab s;
  s.add(0, 3, 1), s.add(0, 3, 1), s.add(0, 9, 1), s.add(1, 0, 1);
  const Order sorted = source_order(s.table(), 0, 4);
  CHECK(sorted.perm.empty() && sorted(2) == 2);
  Table one_file = s.table();
  one_file.file_of = nullptr;
  CHECK(!source_order(one_file, 0, 4).perm.empty());  // offsets 3, 3, 9, 0 of one file
}

static JobSize size_of(const Tab& t, uint64_t slot_max, uint64_t dev_budget) {
  const Table tb = t.table();
  return size_job(tb, source_order(tb, 0, t.n()), 0, t.n(), slot_max, dev_budget);
}

static void test_sizing() {
  const uint64_t slot_max = 512 * kMiB, budget = 16384 * kMiB;
  CHECK(chain_bytes_in_flight(0) == 100000 && chain_bytes_in_flight(64 * 1000) == 50100000);
  {  // the union of runs: overlap counted once, a joined gap counted
    Tab t;
    t.add(0, 0, 100), t.add(0, 50, 100), t.add(0, 150 + kJoinGap, 10), t.add(1, 0, 7), t.add(0, 99, 0);
    const JobSize js = size_of(t, slot_max, budget);
    CHECK(js.bytes == 100 + 50 + kJoinGap + 10 + 7 && js.largest == 100 && js.per == js.bytes);
    CHECK(js.dev_cap == 4096 * kMiB);
  }
  Tab t;  // 1 KiB chunks, contiguous
  for (uint64_t k = 0; k < 32 * 1024; ++k) t.add(0, 1024 * k, 1024);
  CHECK(size_of(t, slot_max, budget).bytes == 32 * kMiB && size_of(t, slot_max, budget).per == 32 * kMiB);
  t.add(0, 32 * kMiB, 1024);  // just above kSplitMin: kSplitMin still beats a quarter
  CHECK(size_of(t, slot_max, budget).per == 32 * kMiB);
  for (uint64_t k = 32 * 1024 + 1; k < 160 * 1024; ++k) t.add(0, 1024 * k, 1024);
  CHECK(size_of(t, slot_max, budget).bytes == 160 * kMiB && size_of(t, slot_max, budget).per == 40 * kMiB);
  CHECK(size_of(t, 36 * kMiB, budget).per == 36 * kMiB);  // capped at slot_max
  {  // never below the largest chunk: 48 MiB of a 64 MiB job
    Tab big;
    big.add(0, 0, 48 * kMiB);
    for (uint64_t k = 0; k < 16; ++k) big.add(0, (48 + k) * kMiB, kMiB);
    const JobSize js = size_of(big, slot_max, budget);
    CHECK(js.bytes == 64 * kMiB && js.largest == 48 * kMiB && js.per == 48 * kMiB);
  }
  {  // long chains: 40 chunks of 3 MiB with 4 MiB slots.  A chain's bytes in flight are
     // 50e3 * (3 MiB / 64 + 2) = 2,457,700,000 > 3 * 4 MiB, a third of them far above both bounds
    Tab chain;
    for (uint64_t k = 0; k < 40; ++k) chain.add(0, 3 * kMiB * k, 3 * kMiB);
    chain.add(0, 1000 * kMiB, 5 * kMiB);  // sz + 15 > slot_max: stays out of the sums
    CHECK(chain_bytes_in_flight(3 * kMiB) == 2457700000ull);
    const JobSize capped = size_of(chain, 4 * kMiB, 64 * kMiB);  // bounded by dev_cap = a quarter of the budget
    CHECK(capped.bytes == 120 * kMiB && capped.largest == 3 * kMiB && capped.dev_cap == 16 * kMiB);
    CHECK(capped.per == 16 * kMiB);
    const JobSize quarter = size_of(chain, 4 * kMiB, 1024 * kMiB);  // bounded by a quarter of the job
    CHECK(quarter.dev_cap == 256 * kMiB && quarter.per == 30 * kMiB);
    CHECK(size_of(chain, 4 * kMiB, kMiB).dev_cap == 4 * kMiB && size_of(chain, 4 * kMiB, kMiB).per == 4 * kMiB);
  }
}

static void test_pieces_and_header() {
  const std::vector<Run> plan{Run{1000, 300, 8, 0, 0}, Run{9000, 100, 320, 0, 1}};
  {  // a run crossing a piece boundary is cut in two
    std::vector<Run> runs = plan;
    PieceCutter c(runs.size());
    c.cut(runs, 0, 256);
    CHECK(c.parts.size() == 1 && c.parts[0].src == 1000 && c.parts[0].len == 248 && c.parts[0].dst == 8);
    c.parts[0].avail = 248;
    c.fold(runs);
    c.cut(runs, 256, 512);
    CHECK(c.parts.size() == 2 && c.part_of == std::vector<size_t>({0, 1}));
    CHECK(c.parts[0].src == 1248 && c.parts[0].len == 52 && c.parts[0].dst == 0 && c.parts[0].file == 0);
    CHECK(c.parts[1].src == 9000 && c.parts[1].len == 100 && c.parts[1].dst == 64 && c.parts[1].file == 1);
    c.parts[0].avail = 52, c.parts[1].avail = 100;
    c.fold(runs);
    CHECK(runs[0].avail == 300 && runs[1].avail == 100);
  }
  {  // after a short part the run's remainder is skipped and avail stops there
    std::vector<Run> runs = plan;
    PieceCutter c(runs.size());
    c.cut(runs, 0, 256);
    c.parts[0].avail = 100;
    c.fold(runs);
    c.cut(runs, 256, 512);
    CHECK(c.parts.size() == 1 && c.part_of[0] == 1 && c.parts[0].src == 9000);
    c.parts[0].avail = 100;
    c.fold(runs);
    CHECK(runs[0].avail == 100 && runs[1].avail == 100);
  }
  Run r{1000, 300, 8, 300, 0};
  HeaderEntry e = header_entry(&r, true, 1100, 50);  // readable
  CHECK(e.ok && e.off == 108 && e.size == 50);
  r.avail = 120;  // short: [1000, 1120) was read
  e = header_entry(&r, true, 1100, 50);
  CHECK(!e.ok && e.off == 0 && e.size == 0);
  e = header_entry(&r, true, 1000, 120);
  CHECK(e.ok && e.off == 8 && e.size == 120);
  e = header_entry(nullptr, true, 5000, 0);  // an empty chunk of an existing file, wherever it lies
  CHECK(e.ok && e.off == 0 && e.size == 0);
  e = header_entry(nullptr, false, 0, 0);  // ... and of a missing one
  CHECK(!e.ok && e.off == 0 && e.size == 0);
}

static bool cover(const std::vector<uint64_t>& o, const std::vector<uint32_t>& s, uint64_t min_span, uint64_t& lo,
                  uint64_t& hi) {
  return gap_free_cover(o.data(), s.data(), o.size(), min_span, lo, hi);
}

static void test_cover_and_slots() {
  uint64_t lo = 0, hi = 0;
  CHECK(cover({10, 110, 210}, {100, 100, 100}, 300, lo, hi) && lo == 10 && hi == 310);
  CHECK(!cover({10, 110, 210}, {100, 100, 100}, 301, lo, hi));  // below the bar
  CHECK(cover({0, 0, 100}, {100, 100, 100}, 1, lo, hi) && lo == 0 && hi == 200);  // a repeated chunk
  CHECK(!cover({0, 0, 200}, {100, 100, 100}, 1, lo, hi));  // ... counts once: [100, 200) is a gap
  CHECK(!cover({0, 100, 201}, {100, 100, 100}, 1, lo, hi));  // one gap of a byte
  CHECK(cover({200, 0, 100, 50}, {100, 100, 100, 0}, 1, lo, hi) && lo == 0 && hi == 300);  // unsorted
  CHECK(!cover({200, 0, 0}, {100, 100, 100}, 1, lo, hi));  // unsorted, repeated, with a gap
  CHECK(!cover({5, 9}, {0, 0}, 0, lo, hi));  // nothing to cover

  std::vector<SlotRun> runs;
  const uint64_t off[] = {10, 0, 31, 50}, len[] = {10, 10, 10, 0};
  CHECK(slot_runs(off, len, 4, runs) == kNoSlot);  // touching slots merge, separate ones do not
  CHECK(runs.size() == 2 && runs[0].lo == 0 && runs[0].hi == 20 && runs[1].lo == 31 && runs[1].hi == 41);
  const uint64_t off2[] = {0, 9}, len2[] = {10, 5};
  CHECK(slot_runs(off2, len2, 2, runs) == 1);  // overlapping: the offending index
  const uint64_t off3[] = {9, 0}, len3[] = {5, 10};
  CHECK(slot_runs(off3, len3, 2, runs) == 0);
}

// ---- property loop ------------------------------------------------------------
static constexpr uint64_t kFileLen[2] = {6200, 3000};  // file 1 is short: reads past 3000 come back short
static uint8_t source_byte(uint32_t file, uint64_t x) { return (uint8_t)(x * 131 + (x >> 8) * 7 + file * 17 + 1); }
static uint64_t emulate_read(uint8_t* dst, const Run& r) {
  const uint64_t flen = kFileLen[r.file], got = r.src >= flen ? 0 : std::min(r.len, flen - r.src);
  for (uint64_t k = 0; k < got; ++k) dst[k] = source_byte(r.file, r.src + k);
  return got;
}

static void check_group(const Tab& t, const Order& order, Group& g, bool in_pieces) {
  CHECK(g.end > g.begin && g.end <= t.n() && g.end - g.begin <= kCap && g.run_of.size() == g.end - g.begin);
  uint64_t edge = 0;
  for (const Run& r : g.runs) {
    CHECK(r.len > 0 && r.dst >= edge && r.dst % 16 == r.src % 16);
    edge = r.dst + r.len;
  }
  CHECK(g.cursor == edge && g.cursor <= kSlot);
  std::vector<uint8_t> slot(kSlot, 0xEE);
  if (in_pieces) {  // the staged route, 200-byte host slots
    PieceCutter c(g.runs.size());
    for (uint64_t p = 0; p < g.cursor; p += 200) {
      c.cut(g.runs, p, std::min(g.cursor, p + 200));
      for (Run& part : c.parts) part.avail = emulate_read(slot.data() + p + part.dst, part);
      c.fold(g.runs);
    }
  } else {
    for (Run& r : g.runs) r.avail = emulate_read(slot.data() + r.dst, r);
  }
  for (uint64_t q = 0; q < g.end - g.begin; ++q) {
    const uint64_t k = order(g.begin + q), o = t.o[k];
    const uint32_t sz = t.s[k], r = g.run_of[q];
    CHECK((r == UINT32_MAX) == (sz == 0));
    const HeaderEntry e = header_entry(r == UINT32_MAX ? nullptr : &g.runs[r], true, o, sz);
    CHECK(e.ok == (sz == 0 || o + sz <= kFileLen[t.f[k]]));
    if (!e.ok) continue;
    CHECK(e.size == sz && e.off + sz <= g.cursor);
    for (uint32_t b = 0; b < sz; ++b)
      if (slot[e.off + b] != source_byte(t.f[k], o + b)) {
        CHECK(!"chunk bytes at the header offset differ from the source");
        break;
      }
  }
}

static void test_random_tables() {
  std::mt19937_64 rng(20240607);
  for (int round = 0; round < 4000; ++round) {
    Tab t;
    const uint64_t n = 1 + rng() % 12;
    uint64_t at = rng() % 64;
    const bool in_order = round % 2 == 0;
    for (uint64_t k = 0; k < n; ++k) {
      const unsigned kind = rng() % 8;
      const uint32_t sz = kind == 0 ? 0 : kind == 1 ? 900 + rng() % 200 : 1 + rng() % 300;
      const uint64_t o = in_order ? at : rng() % 5000;
      t.add(in_order ? (uint32_t)(k >= n / 2) : (uint32_t)(rng() % 2), o, sz);
      if (in_order && k + 1 == n / 2) at = 0;  // the second file starts over
      else if (rng() % 4 == 0) at = o + sz + rng() % 9000;  // a gap, sometimes under kJoinGap
      else at = o + (rng() % 3 ? sz : sz / 2);  // contiguous or overlapping
    }
    const Table tb = t.table();
    const Order order = source_order(tb, 0, n);
    CHECK(!in_order || order.perm.empty());
    for (uint64_t q = 1; q < n; ++q) {
      const uint64_t a = order(q - 1), b = order(q);
      CHECK(t.f[a] < t.f[b] || (t.f[a] == t.f[b] && t.o[a] <= t.o[b]));
    }
    Group g;
    for (uint64_t i = 0; i < n; i = g.end) {  // groups partition [0, n) in order
      pack_group(tb, order, i, n, kSlot, kCap, g);
      CHECK(g.begin == i);
      if (g.oversize) {
        CHECK(g.end == i + 1 && (uint64_t)t.s[order(i)] + 15 > kSlot);
        continue;
      }
      check_group(t, order, g, round % 4 >= 2);
      if (g.end <= i) return;  // reported above; do not spin
    }
  }
}

int main() {
  test_runs();
  test_group_ends();
  test_order();
  test_sizing();
  test_pieces_and_header();
  test_cover_and_slots();
  test_random_tables();
  if (g_failed) {
    printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("stage_plan_tests: OK\n");
  return 0;
}
