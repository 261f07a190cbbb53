// update_plan_tests.cpp -- the planner of lbf_sha1_update_batch
// (bitflood_amd/csrc/update_plan.hpp) on the CPU: every refusal, the cutting
// of a call into launches, and the packing of a launch into copies.  Includes
// only that header and links nothing; tests/test_update_cpu.py compiles it with
// plain g++ and again with -fsanitize=address,undefined and runs both.
#include "update_plan.hpp"

#include "check_cases.hpp"

#include <cstdio>
#include <cstring>

using namespace lbf;

static int g_fail = 0;
#define CHECK(cond)                                                                \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      std::fprintf(stderr, "%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                                    \
    }                                                                              \
  } while (0)

static std::vector<lbf_sha1_state> fresh(size_t n) {
  std::vector<lbf_sha1_state> s(n);
  std::memset(s.data(), 0, n * sizeof(lbf_sha1_state));
  return s;
}

static void test_refusals() {
  std::string why;
  std::vector<lbf_sha1_state> st = fresh(4);
  const uint64_t offs[3] = {0, 100, 200};
  const uint32_t sizes[3] = {100, 100, 56};
  const uint32_t so[3] = {2, 0, 3};
  CHECK(update_check(st.data(), 4, so, 256, offs, sizes, 3, why) == kNoPiece);
  CHECK(update_check(st.data(), 4, nullptr, 256, offs, sizes, 3, why) == kNoPiece);
  // a piece outside [base, base + base_len): past the end, and an offset past the end with size 0 allowed at the end
  CHECK(update_check(st.data(), 4, so, 255, offs, sizes, 3, why) == 2 && why.find("outside") != std::string::npos);
  const uint64_t far[1] = {UINT64_MAX};
  const uint32_t one[1] = {1};
  CHECK(update_check(st.data(), 4, nullptr, 256, far, one, 1, why) == 0);
  const uint64_t at_end[1] = {256};
  const uint32_t zero[1] = {0};
  CHECK(update_check(st.data(), 4, nullptr, 256, at_end, zero, 1, why) == kNoPiece);
  // a state index >= n_states, named or implied
  const uint32_t so_bad[3] = {2, 4, 3};
  CHECK(update_check(st.data(), 4, so_bad, 256, offs, sizes, 3, why) == 1 && why.find("state 4") != std::string::npos);
  CHECK(update_check(st.data(), 2, nullptr, 256, offs, sizes, 3, why) == 2);
  // two pieces of one state: the later one is named
  const uint32_t so_dup[3] = {3, 0, 3};
  CHECK(update_check(st.data(), 4, so_dup, 256, offs, sizes, 3, why) == 2 && why.find("second piece") != std::string::npos);
  // corrupt states: buffered > 63, buffered != total % 64
  st[0].buffered = 64;
  st[0].total = 64;
  CHECK(update_check(st.data(), 4, so, 256, offs, sizes, 3, why) == 1 && why.find("corrupt") != std::string::npos);
  st[0].buffered = 5;
  st[0].total = 70;
  CHECK(update_check(st.data(), 4, so, 256, offs, sizes, 3, why) == 1);
  st[0].total = 69;
  CHECK(update_check(st.data(), 4, so, 256, offs, sizes, 3, why) == kNoPiece);
  // total + size past 2^61
  st[0].buffered = 28;
  st[0].total = kUpdateMaxTotal - 100;
  CHECK(update_check(st.data(), 4, so, 256, offs, sizes, 3, why) == kNoPiece);  // exactly 2^61
  st[0].buffered = 0;
  st[0].total = kUpdateMaxTotal - 64;
  CHECK(update_check(st.data(), 4, so, 256, offs, sizes, 3, why) == 1 && why.find("2^61") != std::string::npos);
  st[0].total = UINT64_MAX - 63;
  CHECK(update_check(st.data(), 4, so, 256, offs, sizes, 3, why) == 1);
  // an untouched corrupt state does not matter
  st[0].total = 0;
  st[1].buffered = 99;
  CHECK(update_check(st.data(), 4, so, 256, offs, sizes, 3, why) == kNoPiece);
}

// Every property of a plan: each piece's cuts cover it in order without a gap,
// fall on 64-byte multiples of the piece, never share a launch, only the last
// is marked; no launch carries more than the cap (a multiple of 64, at least 64).
static void check_plan(const std::vector<uint64_t>& offs, const std::vector<uint32_t>& sizes, uint64_t cap,
                       size_t want_launches) {
  const std::vector<std::vector<UpdateCut>> plan = update_launches(offs.data(), sizes.data(), offs.size(), cap);
  std::vector<uint64_t> done(offs.size(), 0);
  std::vector<bool> ended(offs.size(), false);
  std::vector<long> last_launch(offs.size(), -1);
  uint64_t next_piece = 0;
  for (size_t l = 0; l < plan.size(); ++l) {
    uint64_t bytes = 0;
    for (const UpdateCut& c : plan[l]) {
      CHECK(c.piece < offs.size());
      CHECK(!ended[c.piece]);
      CHECK(c.off == offs[c.piece] + done[c.piece]);  // in order, no gap
      CHECK(done[c.piece] % 64 == 0);                 // cut at a 64-byte multiple of the piece
      CHECK(last_launch[c.piece] < (long)l);          // cuts of one piece never share a launch
      if (done[c.piece] == 0) {
        CHECK(c.piece == next_piece);  // pieces in caller order
        ++next_piece;
      }
      last_launch[c.piece] = (long)l;
      done[c.piece] += c.size;
      CHECK(c.last == (done[c.piece] == sizes[c.piece]));
      if (c.last) ended[c.piece] = true;
      bytes += c.size;
    }
    CHECK(bytes <= std::max<uint64_t>(64, cap & ~63ull));  // the cap as the planner rounds it
    CHECK(!plan[l].empty() || plan.size() == 1);
  }
  for (size_t i = 0; i < offs.size(); ++i) CHECK(ended[i] && done[i] == sizes[i]);
  CHECK(plan.size() == want_launches);
}

static void test_cutting() {
  const uint64_t MiB = 1 << 20;
  // the issue's pieces under a 1 MiB cap, one call
  std::vector<uint32_t> sizes = {0, 1, 64, (uint32_t)MiB - 1, (uint32_t)MiB, (uint32_t)MiB + 65, 3 * (uint32_t)MiB};
  std::vector<uint64_t> offs;
  uint64_t at = 7;
  for (uint32_t s : sizes) {
    offs.push_back(at);
    at += s;
  }
  // launches: {0, 1, 64, MiB-1 does not fit -> next}, {MiB-1}, {MiB}, {MiB+65: MiB | 65}, {3 MiB: MiB-128 | MiB | MiB | 128}
  //   = [0,1,64] [MiB-1] [MiB] [cut MiB] [65, cut MiB-128 (room floor64(MiB-65))] [MiB] [MiB] [128]
  check_plan(offs, sizes, MiB, 8);
  // each alone
  for (size_t k = 0; k < sizes.size(); ++k) {
    const size_t want = sizes[k] <= MiB ? 1 : (sizes[k] + MiB - 1) / MiB;
    check_plan({offs[k]}, {sizes[k]}, MiB, want);
  }
  // a cap that is no multiple of 64 is rounded down; tiny caps still make progress
  check_plan({0}, {1000}, 200, 6);  // 192-byte launches: 5 full + 40
  check_plan({0, 1000}, {1000, 30}, 1, 17);  // 64-byte launches: 15 full + 40, then 30 no longer fits beside the 40
  // nothing to do
  CHECK(update_launches(nullptr, nullptr, 0, MiB).size() == 1);
  // many small pieces fill launches without cutting
  std::vector<uint64_t> o2;
  std::vector<uint32_t> s2;
  for (int k = 0; k < 100; ++k) o2.push_back(k * 40000ull), s2.push_back(40000);
  check_plan(o2, s2, MiB, 4);  // 26 pieces per launch
  for (const auto& l : update_launches(o2.data(), s2.data(), 100, MiB))
    for (const UpdateCut& c : l) CHECK(c.last && c.size == 40000);
}

static void test_runs() {
  // adjacent pieces travel in one copy; a gap starts another at the source's 16-byte phase; empty pieces take none
  std::vector<UpdateCut> cuts = {{0, 5, 100, true},   {1, 105, 0, true},  {2, 105, 50, true},
                                 {3, 1000, 10, true}, {4, 155, 5, true}, {5, 1003, 20, true}};
  std::vector<Run> runs;
  std::vector<uint64_t> dev;
  const uint64_t area = update_runs(cuts, runs, dev);
  CHECK(runs.size() == 4);
  CHECK(runs[0].src == 5 && runs[0].len == 150 && runs[0].dst % 16 == 5);
  CHECK(runs[1].src == 1000 && runs[1].len == 10 && runs[1].dst % 16 == 1000 % 16 && runs[1].dst >= runs[0].dst + 150);
  CHECK(runs[2].src == 155 && runs[2].len == 5 && runs[2].dst % 16 == 155 % 16 && runs[2].dst >= runs[1].dst + 10);
  // 1003 lies inside run 1, but only the current run is extended
  CHECK(runs[3].src == 1003 && runs[3].len == 20 && runs[3].dst % 16 == 1003 % 16 && runs[3].dst >= runs[2].dst + 5);
  CHECK(dev[0] == runs[0].dst && dev[2] == runs[0].dst + 100 && dev[3] == runs[1].dst && dev[4] == runs[2].dst &&
        dev[5] == runs[3].dst);
  CHECK(area == runs[3].dst + 20);
  // only pieces' bytes are read: no gap is copied along
  uint64_t sum = 0;
  for (const Run& r : runs) sum += r.len;
  CHECK(sum == 100 + 50 + 10 + 5 + 20);
  // a piece that starts inside the current run shares its bytes
  std::vector<UpdateCut> over = {{0, 64, 100, true}, {1, 100, 100, true}};
  update_runs(over, runs, dev);
  CHECK(runs.size() == 1 && runs[0].len == 136 && dev[1] == dev[0] + 36);
}

// Sources on both sides of byte 2^32 of the caller's buffer: three pieces that
// touch one another across the line, and one past 3 * 2^32.  Nothing in the
// plan may be kept in 32 bits.
static void test_past_4gib() {
  const uint64_t G = 1ull << 32;
  const std::vector<uint64_t> offs = {G - 70, G - 6, G + 64, 3 * G + 5};
  const std::vector<uint32_t> sizes = {64, 70, 100, 33};
  const uint64_t end = 3 * G + 5 + 33;
  std::string why;
  std::vector<lbf_sha1_state> st = fresh(4);
  // bounds: exactly at the last piece's end, one byte short of it, and a buffer that ends at the line
  CHECK(update_check(st.data(), 4, nullptr, end, offs.data(), sizes.data(), 4, why) == kNoPiece);
  CHECK(update_check(st.data(), 4, nullptr, end - 1, offs.data(), sizes.data(), 4, why) == 3 &&
        why.find("outside") != std::string::npos);
  CHECK(update_check(st.data(), 4, nullptr, G, offs.data(), sizes.data(), 4, why) == 1);
  CHECK(update_check(st.data(), 4, nullptr, G + 64, offs.data(), sizes.data(), 3, why) == 2);
  CHECK(update_check(st.data(), 4, nullptr, G + 164, offs.data(), sizes.data(), 3, why) == kNoPiece);
  // a base_len whose low 32 bits are large enough and whose high bits are not
  CHECK(update_check(st.data(), 4, nullptr, (uint32_t)end + 2 * G, offs.data(), sizes.data(), 4, why) == 3);
  // one launch, the cuts at the 64-bit offsets
  check_plan(offs, sizes, 1 << 20, 1);
  const std::vector<std::vector<UpdateCut>> plan = update_launches(offs.data(), sizes.data(), 4, 1 << 20);
  CHECK(plan.size() == 1 && plan[0].size() == 4);
  for (size_t k = 0; k < 4 && k < plan[0].size(); ++k)
    CHECK(plan[0][k].off == offs[k] && plan[0][k].size == sizes[k] && plan[0][k].last);
  // a piece cut into launches keeps counting past the line: 64-byte launches from 2^32 - 70
  const std::vector<std::vector<UpdateCut>> cut = update_launches(offs.data(), sizes.data(), 2, 64);
  CHECK(cut.size() == 3);
  if (cut.size() == 3) {
    CHECK(cut[0].size() == 1 && cut[0][0].off == G - 70 && cut[0][0].size == 64);
    CHECK(cut[1].size() == 1 && cut[1][0].off == G - 6 && cut[1][0].size == 64 && !cut[1][0].last);
    CHECK(cut[2].size() == 1 && cut[2][0].off == G + 58 && cut[2][0].size == 6 && cut[2][0].last);
  }
  // the runs join across the line; device positions keep the source's phase mod 16
  std::vector<Run> runs;
  std::vector<uint64_t> dev;
  const uint64_t area = update_runs(plan[0], runs, dev);
  CHECK(runs.size() == 2);
  if (runs.size() == 2) {
    CHECK(runs[0].src == G - 70 && runs[0].len == 234 && runs[0].dst % 16 == (G - 70) % 16);
    CHECK(runs[1].src == 3 * G + 5 && runs[1].len == 33 && runs[1].dst % 16 == 5 && runs[1].dst >= runs[0].dst + 234);
    CHECK(dev[0] == runs[0].dst && dev[1] == dev[0] + 64 && dev[2] == dev[0] + 134 && dev[3] == runs[1].dst);
    CHECK(area == runs[1].dst + 33 && area < 512);
  }
  for (size_t k = 0; k < 4; ++k) CHECK(dev[k] % 16 == offs[k] % 16);
  // out of order: a piece below the line after one above it starts a run of its own
  std::vector<UpdateCut> back = {{0, G + 64, 100, true}, {1, G - 6, 70, true}, {2, G + 164, 8, true}};
  update_runs(back, runs, dev);
  CHECK(runs.size() == 3 && runs[1].src == G - 6 && runs[1].dst % 16 == (G - 6) % 16 && runs[2].src == G + 164);
}

// The one-piece and the seq checker over seeded calls (check_cases.hpp): each
// answers what tests/golden/plan_checks.txt records of the checkers before the
// planners were merged, and where no state repeats the two agree to the word.
static void test_checkers_agree() {
  using namespace plan_cases;
  const std::vector<Recorded> want = read_fixture(fixture_path(__FILE__));
  CHECK(want.size() == kCases);
  if (want.size() != kCases) return;
  uint64_t repeats = 0, refused = 0;
  for (uint64_t k = 0; k < kCases; ++k) {
    const Case c = make_case(k);
    CHECK(checksum(c) == want[k].sum);
    Answer one, seq;
    one.piece = update_check(c.states.data(), c.n_states, c.so(), c.base_len, c.offsets.data(), c.sizes.data(), c.n,
                             one.why);
    seq.piece = update_seq_check(c.states.data(), c.n_states, c.so(), c.base_len, c.offsets.data(), c.sizes.data(),
                                 nullptr, c.n, seq.why);
    CHECK(one == want[k].hash_one);
    CHECK(seq == want[k].hash_seq);
    if (!c.repeats) CHECK(one == seq);
    repeats += c.repeats;
    refused += one.piece != kNoPiece;
  }
  CHECK(repeats > kCases / 4 && repeats < kCases / 2 && refused > kCases / 4);
}

// The one-piece calls' chain table: for ids of which none repeats, the identity equals the grouping.
static void test_identity_table() {
  const std::vector<std::vector<uint64_t>> cases = {{}, {0}, {7, 3, 9, 0}, {1ull << 32, 0, 5}, {4, 3, 2, 1, 0}};
  for (const std::vector<uint64_t>& ids : cases) {
    const ChainTable a = identity_table(ids), b = chain_table(ids);
    CHECK(a.order == b.order && a.chain_id == b.chain_id && a.first == b.first && a.chains() == ids.size());
  }
  std::vector<uint64_t> many(1000);
  for (size_t k = 0; k < many.size(); ++k) many[k] = (k * 7919) % 1000 + (k % 3 ? 0 : 1ull << 40);
  const ChainTable a = identity_table(many), b = chain_table(many);
  CHECK(a.order == b.order && a.chain_id == b.chain_id && a.first == b.first);
  // by a launch's cuts: the state each cut's piece names, or the piece itself
  const uint32_t so[3] = {5, 2, 9};
  const std::vector<UpdateCut> cuts = {UpdateCut{2, 0, 8, true}, UpdateCut{0, 8, 8, true}};
  CHECK((table_of(cuts, so, false).chain_id == std::vector<uint64_t>{9, 5}));
  CHECK((table_of(cuts, nullptr, false).chain_id == std::vector<uint64_t>{2, 0}));
  CHECK((table_of(cuts, so, true).chain_id == std::vector<uint64_t>{9, 5}));
}

// Where a hash launch's tables lie: the numbers of the hand-written offset
// chains the layout replaced.  One piece per state: states (96 m) | offsets
// (8 m) | sizes (4 m) | expected (20 m) | final flags (m).  Seq: states (96 nc)
// | offsets (8 m) | chain_first (4 (nc + 1)) | sizes | expected | final flags.
static void test_table_offsets() {
  struct One { uint64_t m, off, size, exp, fin, bytes; };
  const One one[3] = {{1, 96, 104, 108, 128, 129}, {2, 192, 208, 216, 256, 258}, {7, 672, 728, 756, 896, 903}};
  for (const One& w : one) {
    const HashTables t = hash_tables(w.m, w.m, false);
    CHECK(t.states == 0 && t.off == w.off && t.size == w.size && t.exp == w.exp && t.fin == w.fin &&
          t.bytes == w.bytes);
  }
  struct Seq { uint64_t m, nc, off, first, size, exp, fin, bytes; };
  const Seq seq[5] = {{1, 1, 96, 104, 112, 116, 136, 137},
                      {2, 1, 96, 112, 120, 128, 168, 170},
                      {2, 2, 192, 208, 220, 228, 268, 270},
                      {7, 1, 96, 152, 160, 188, 328, 335},
                      {7, 7, 672, 728, 760, 788, 928, 935}};
  for (const Seq& w : seq) {
    const HashTables t = hash_tables(w.m, w.nc, true);
    CHECK(t.states == 0 && t.off == w.off && t.first == w.first && t.size == w.size && t.exp == w.exp &&
          t.fin == w.fin && t.bytes == w.bytes);
  }
  CHECK(round_up(0, 256) == 0 && round_up(1, 256) == 256 && round_up(256, 256) == 256 && round_up(257, 256) == 512);
}

int main() {
  test_refusals();
  test_cutting();
  test_runs();
  test_past_4gib();
  test_checkers_agree();
  test_identity_table();
  test_table_offsets();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("update_plan_tests: OK\n");
  return 0;
}
