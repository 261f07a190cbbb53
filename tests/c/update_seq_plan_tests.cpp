// update_seq_plan_tests.cpp -- the planner of lbf_sha1_update_seq_batch and
// lbf_b64_update_seq_batch (bitflood_amd/csrc/update_plan.hpp, b64_update_plan.hpp) on the CPU:
// the stable grouping into a chain table, chains that straddle launches, every
// refusal, and the text areas and copy-back ranges of a chain.  Includes only
// those headers and links nothing; tests/test_update_seq_cpu.py compiles it with
// plain g++ and again with -fsanitize=address,undefined and runs both.
#include "b64_update_plan.hpp"

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

static std::vector<lbf_b64_state> fresh_b64(size_t n) {
  std::vector<lbf_b64_state> s(n);
  std::memset(s.data(), 0, n * sizeof(lbf_b64_state));
  return s;
}

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

static void test_grouping() {
  // no state repeats: the identity, chain c = item c
  {
    const ChainTable t = chain_table({7, 3, 9, 0});
    CHECK((t.order == std::vector<uint32_t>{0, 1, 2, 3}));
    CHECK((t.chain_id == std::vector<uint64_t>{7, 3, 9, 0}));
    CHECK((t.first == std::vector<uint32_t>{0, 1, 2, 3, 4}));
    CHECK(t.chains() == 4);
  }
  // repeats: chains in the order of their first items, items in their own order
  {
    const ChainTable t = chain_table({5, 2, 5, 7, 2, 5});
    CHECK((t.order == std::vector<uint32_t>{0, 2, 5, 1, 4, 3}));
    CHECK((t.chain_id == std::vector<uint64_t>{5, 2, 7}));
    CHECK((t.first == std::vector<uint32_t>{0, 3, 5, 6}));
  }
  // one chain, and nothing
  {
    const ChainTable t = chain_table({4, 4, 4});
    CHECK((t.order == std::vector<uint32_t>{0, 1, 2}) && t.chains() == 1 && (t.first == std::vector<uint32_t>{0, 3}));
    const ChainTable e = chain_table({});
    CHECK(e.order.empty() && e.chains() == 0 && (e.first == std::vector<uint32_t>{0}));
  }
  // ids past 2^32 stay apart
  {
    const ChainTable t = chain_table({1ull << 32, 0, 1ull << 32});
    CHECK((t.order == std::vector<uint32_t>{0, 2, 1}) && t.chains() == 2 && t.chain_id[0] == 1ull << 32);
  }
}

// The chain table of one launch's cuts, as update_batch.cpp builds it for the seq calls.
static ChainTable table_of(const std::vector<UpdateCut>& cuts, const uint32_t* state_of) {
  return table_of(cuts, state_of, true);
}

static void test_straddling() {
  // six pieces of 64 bytes, states 0 1 0 1 0 1, launches of 128 bytes: every launch holds one piece of each chain
  {
    const uint64_t offs[6] = {0, 64, 128, 192, 256, 320};
    const uint32_t sizes[6] = {64, 64, 64, 64, 64, 64};
    const uint32_t so[6] = {0, 1, 0, 1, 0, 1};
    const auto launches = update_launches(offs, sizes, 6, 128);
    CHECK(launches.size() == 3);
    uint64_t next = 0;
    for (const auto& cuts : launches) {
      CHECK(cuts.size() == 2);
      const ChainTable t = table_of(cuts, so);
      CHECK(t.chains() == 2 && t.chain_id[0] == 0 && t.chain_id[1] == 1);
      for (const UpdateCut& c : cuts) CHECK(c.piece == next++ && c.last);  // caller order over the launches
    }
  }
  // launches of 192 bytes: chain 0 has two pieces in the first launch and one in the second
  {
    const uint64_t offs[6] = {0, 64, 128, 192, 256, 320};
    const uint32_t sizes[6] = {64, 64, 64, 64, 64, 64};
    const uint32_t so[6] = {0, 1, 0, 1, 0, 1};
    const auto launches = update_launches(offs, sizes, 6, 192);
    CHECK(launches.size() == 2);
    const ChainTable a = table_of(launches[0], so), b = table_of(launches[1], so);
    CHECK((a.order == std::vector<uint32_t>{0, 2, 1}) && (a.first == std::vector<uint32_t>{0, 2, 3}));
    CHECK((b.order == std::vector<uint32_t>{0, 2, 1}) && (b.chain_id == std::vector<uint64_t>{1, 0}));
    CHECK((b.first == std::vector<uint32_t>{0, 2, 3}));
  }
  // a piece larger than a launch between two small ones of the same chain: its cuts never share a launch, so
  // no launch holds two cuts of it, and the chain's order over the launches is the caller's
  {
    const uint64_t offs[3] = {0, 10, 1000};
    const uint32_t sizes[3] = {10, 300, 7};
    const uint32_t so[3] = {4, 4, 4};
    const auto launches = update_launches(offs, sizes, 3, 128);
    uint64_t at = 0, last_piece = 0;
    size_t cuts_of_big = 0;
    for (const auto& cuts : launches) {
      const ChainTable t = table_of(cuts, so);
      CHECK(t.chains() == 1 && t.chain_id[0] == 4);
      size_t big_here = 0;
      for (size_t k = 0; k < cuts.size(); ++k) {
        CHECK(t.order[k] == k);  // one chain: table order is launch order
        CHECK(cuts[k].piece >= last_piece);
        last_piece = cuts[k].piece;
        if (cuts[k].piece == 1) {
          CHECK(cuts[k].off == 10 + at);
          at += cuts[k].size;
          CHECK(cuts[k].last == (at == 300));
          ++big_here;
          ++cuts_of_big;
        }
      }
      CHECK(big_here <= 1);
    }
    CHECK(at == 300 && cuts_of_big >= 3);
    CHECK(launches.front().front().piece == 0 && launches.back().back().piece == 2);
  }
}

static void test_hash_refusals() {
  std::string why;
  std::vector<lbf_sha1_state> st = fresh(4);
  const uint64_t offs[4] = {0, 100, 200, 50};
  const uint32_t sizes[4] = {100, 100, 56, 10};
  const uint32_t so[4] = {2, 0, 2, 2};  // three pieces of state 2: accepted here
  const uint8_t none[4] = {0, 0, 0, 0};
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, none, 4, why) == kNoPiece);
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, nullptr, 4, why) == kNoPiece);
  CHECK(update_seq_check(st.data(), 4, nullptr, 256, offs, sizes, nullptr, 4, why) == kNoPiece);
  // what update_check refuses
  CHECK(update_seq_check(st.data(), 4, so, 255, offs, sizes, none, 4, why) == 2 && has(why, "outside"));
  const uint64_t far[1] = {UINT64_MAX};
  const uint32_t one[1] = {1};
  CHECK(update_seq_check(st.data(), 4, nullptr, 256, far, one, nullptr, 1, why) == 0);
  const uint32_t so_bad[4] = {2, 4, 2, 2};
  CHECK(update_seq_check(st.data(), 4, so_bad, 256, offs, sizes, none, 4, why) == 1 && has(why, "state 4"));
  CHECK(update_seq_check(st.data(), 3, nullptr, 256, offs, sizes, none, 4, why) == 3);
  st[2].buffered = 64;
  st[2].total = 64;
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, none, 4, why) == 0 && has(why, "corrupt"));
  st[2].buffered = 5;
  st[2].total = 70;
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, none, 4, why) == 0);
  st[2].total = 69;
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, none, 4, why) == kNoPiece);
  // total plus the SUM of the chain's sizes past 2^61: 100 + 56 + 10 = 166 for state 2
  st[2].buffered = (uint32_t)((kUpdateMaxTotal - 166) % 64);
  st[2].total = kUpdateMaxTotal - 166;
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, none, 4, why) == kNoPiece);  // exactly 2^61
  st[2].buffered = (uint32_t)((kUpdateMaxTotal - 165) % 64);
  st[2].total = kUpdateMaxTotal - 165;
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, none, 4, why) == 3 && has(why, "2^61"));  // the last one
  st[2].buffered = (uint32_t)((kUpdateMaxTotal - 110) % 64);
  st[2].total = kUpdateMaxTotal - 110;
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, none, 4, why) == 2 && has(why, "2^61"));  // each alone fits
  st[2].buffered = 0;
  st[2].total = UINT64_MAX - 63;
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, none, 4, why) == 0);
  st[2].total = 0;
  // a final piece that another piece of its state follows: the final piece is named
  const uint8_t fin_mid[4] = {0, 0, 1, 0};
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, fin_mid, 4, why) == 2 && has(why, "is final") &&
        has(why, "piece 3"));
  const uint8_t fin_first[4] = {1, 1, 0, 1};
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, fin_first, 4, why) == 0 && has(why, "piece 2"));
  // final and last of its state: accepted, whatever follows of other states
  const uint8_t fin_last[4] = {0, 1, 0, 1};
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, fin_last, 4, why) == kNoPiece);
  // an untouched corrupt state does not matter
  st[1].buffered = 99;
  CHECK(update_seq_check(st.data(), 4, so, 256, offs, sizes, fin_last, 4, why) == kNoPiece);
}

static void test_text_refusals() {
  std::string why;
  std::vector<lbf_sha1_state> sha = fresh(3);
  std::vector<lbf_b64_state> b64 = fresh_b64(3);
  // two chains: state 1 (slot [0, 90)) with three pieces, state 0 (slot [100, 130)) with one
  const uint64_t toffs[4] = {0, 40, 80, 120};
  const uint32_t tlens[4] = {40, 40, 40, 40};
  const uint32_t so[4] = {1, 0, 1, 1};
  const uint32_t caps[4] = {90, 30, 90, 90};
  const uint64_t ooffs[4] = {0, 100, 0, 0};
  const uint8_t fin[4] = {0, 1, 0, 1};
  auto check = [&](const uint32_t* s, const uint64_t* to, const uint32_t* tl, const uint8_t* f, const uint32_t* c,
                   uint64_t out_len, const uint64_t* oo) {
    return b64_update_seq_check(b64.data(), sha.data(), 3, s, 160, to, tl, f, 4, c, out_len, oo, why);
  };
  CHECK(check(so, toffs, tlens, fin, caps, 130, ooffs) == kNoPiece);
  CHECK(check(so, toffs, tlens, nullptr, caps, 130, ooffs) == kNoPiece);
  // what b64_update_check refuses
  const uint32_t tl_bad[4] = {40, 40, 40, 41};
  CHECK(check(so, toffs, tl_bad, fin, caps, 130, ooffs) == 3 && has(why, "text outside"));
  const uint32_t cap_big[4] = {90, (1u << 30) + 1, 90, 90};
  CHECK(check(so, toffs, tlens, fin, cap_big, 1ull << 31, ooffs) == 1 && has(why, "1 GiB"));
  CHECK(check(so, toffs, tlens, fin, caps, 129, ooffs) == 1 && has(why, "slot outside"));
  const uint32_t so_bad[4] = {1, 3, 1, 1};
  CHECK(check(so_bad, toffs, tlens, fin, caps, 130, ooffs) == 1 && has(why, "state 3"));
  b64[1].ncarry = 4;
  CHECK(check(so, toffs, tlens, fin, caps, 130, ooffs) == 0 && has(why, "corrupt"));
  b64[1].ncarry = 0;
  b64[1].decoded = 3;  // the SHA state's total is 0
  CHECK(check(so, toffs, tlens, fin, caps, 130, ooffs) == 0 && has(why, "SHA state total"));
  sha[1].total = 3;
  sha[1].buffered = 3;
  CHECK(check(so, toffs, tlens, fin, caps, 130, ooffs) == kNoPiece);
  // pieces of one state that name different slots or chunk sizes
  const uint64_t oo_diff[4] = {0, 100, 0, 1};
  CHECK(check(so, toffs, tlens, fin, caps, 130, oo_diff) == 3 && has(why, "another slot") && has(why, "piece 0"));
  const uint32_t cap_diff[4] = {90, 30, 89, 90};
  CHECK(check(so, toffs, tlens, fin, cap_diff, 130, ooffs) == 2 && has(why, "another slot"));
  // a final piece that another piece of its state follows
  const uint8_t fin_mid[4] = {1, 1, 0, 1};
  CHECK(check(so, toffs, tlens, fin_mid, caps, 130, ooffs) == 0 && has(why, "is final") && has(why, "piece 2"));
  // slots of different states that overlap; the same slot named by one state's pieces does not
  const uint64_t oo_over[4] = {0, 89, 0, 0};
  CHECK(check(so, toffs, tlens, fin, caps, 130, oo_over) == 1 && has(why, "overlaps"));
  const uint64_t oo_touch[4] = {0, 90, 0, 0};
  CHECK(check(so, toffs, tlens, fin, caps, 130, oo_touch) == kNoPiece);
  const uint32_t so_two[4] = {1, 0, 1, 2};  // state 2 names state 1's slot
  CHECK(check(so_two, toffs, tlens, nullptr, caps, 130, ooffs) == 3 && has(why, "overlaps"));
  // empty slots hold nothing
  const uint32_t cap_zero[4] = {90, 0, 90, 90};
  const uint64_t oo_in[4] = {0, 50, 0, 0};
  sha[0].total = 0;
  CHECK(check(so, toffs, tlens, fin, cap_zero, 130, oo_in) == kNoPiece);
}

// One chain of `pieces` pieces of `len` characters each, standing at `decoded` of a chunk of `cap` bytes.
static void one_chain(uint64_t decoded, uint32_t nc, uint32_t pieces, uint32_t len, uint32_t cap, uint64_t want_room) {
  std::vector<B64Place> places;
  const uint64_t chars = (uint64_t)pieces * len;
  const uint64_t area = b64_update_places({decoded}, {nc}, {chars}, {cap}, places);
  const uint64_t at = std::min<uint64_t>(decoded, cap);
  CHECK(places.size() == 1);
  CHECK(places[0].dev == at % 64);                 // the chain's position mod 64: the hash's aligned loop applies
  CHECK(places[0].slot + at == places[0].dev);     // mod 2^64
  CHECK(places[0].room == want_room);
  CHECK(area == places[0].dev + places[0].room);
}

static void test_text_areas() {
  // chains of 1 and 3 pieces that start below the cap, at it and past it
  one_chain(0, 0, 1, 40, 1000, 32);        // 3 * 10 + 2
  one_chain(0, 0, 3, 40, 1000, 92);        // 3 * 30 + 2: one bound over the chain's characters
  one_chain(300, 3, 3, 40, 1000, 92);      // (3 + 120) / 4 = 30 groups
  one_chain(300, 3, 1, 41, 1000, 35);      // (3 + 41) / 4 = 11 groups
  one_chain(990, 0, 1, 40, 1000, 10);      // clipped to what is left of the slot
  one_chain(990, 0, 3, 40, 1000, 10);
  one_chain(1000, 0, 1, 40, 1000, 0);      // at the cap: nothing can be written
  one_chain(1000, 0, 3, 40, 1000, 0);
  one_chain(1002, 0, 3, 40, 1000, 0);      // past it (the decoder counts on)
  one_chain(5, 0, 3, 0, 1000, 2);          // empty pieces
  // two chains in one launch follow one another, each at its position mod 64
  std::vector<B64Place> places;
  const uint64_t area = b64_update_places({3, 130}, {0, 1}, {8, 400}, {90, 1000}, places);
  CHECK(places[0].dev == 3 && places[0].room == 8);
  CHECK(places[1].dev >= places[0].dev + places[0].room && places[1].dev % 64 == 130 % 64 && places[1].dev < 11 + 64);
  CHECK(places[1].room == 3 * 100 + 2 && area == places[1].dev + places[1].room);
  CHECK(places[1].slot + 130 == places[1].dev);
  // copy-back: one range per chain (its pieces decode to adjacent bytes); chains whose ranges touch on both
  // sides travel as one run, a chain that got nothing takes none
  std::vector<Run> runs;
  copyback_runs({places[0].dev, places[1].dev}, {1000 + 3, 5000 + 130}, {6, 300}, runs);
  CHECK(runs.size() == 2 && runs[0].src == 3 && runs[0].dst == 1003 && runs[0].len == 6);
  CHECK(runs[1].src == places[1].dev && runs[1].dst == 5130 && runs[1].len == 300);
  copyback_runs({0, 64, 70}, {100, 200, 206}, {10, 6, 3}, runs);
  CHECK(runs.size() == 2 && runs[1].src == 64 && runs[1].len == 9);
  copyback_runs({0, 64}, {100, 200}, {0, 0}, runs);
  CHECK(runs.empty());
}

int main() {
  test_grouping();
  test_straddling();
  test_hash_refusals();
  test_text_refusals();
  test_text_areas();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("update_seq_plan_tests: OK\n");
  return 0;
}
