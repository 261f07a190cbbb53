// b64_encode_plan_tests.cpp -- the planner of lbf_b64_encode_update_batch
// (bitflood_amd/csrc/b64_encode_plan.hpp) on the CPU: every refusal, the cut of
// an oversized piece, which characters a cut writes, where a launch's
// characters lie on the device and how they come back.  Includes only that
// header and links nothing; tests/test_b64_encode_cpu.py compiles it with plain
// g++ and again with -fsanitize=address,undefined and runs both.
#include "b64_encode_plan.hpp"

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

struct Pairs {
  std::vector<lbf_b64_enc_state> e;
  std::vector<lbf_sha1_state> s;
  explicit Pairs(size_t n) : e(n), s(n) {
    std::memset(e.data(), 0, n * sizeof(lbf_b64_enc_state));
    std::memset(s.data(), 0, n * sizeof(lbf_sha1_state));
  }
  void at(size_t k, uint64_t taken) {  // a consistent pair mid-chunk
    e[k].taken = taken;
    e[k].ncarry = (uint8_t)(taken % 3);
    e[k].carry = taken % 3 == 2 ? 0xBBAAu : taken % 3 == 1 ? 0xAAu : 0u;
    s[k].total = taken;
    s[k].buffered = (uint32_t)(taken % 64);
  }
};

static bool has(const std::string& why, const char* what) { return why.find(what) != std::string::npos; }

static void test_geometry() {
  using namespace b64e;
  CHECK(group_pos(0, false) == 0 && group_pos(17, false) == 68 && group_pos(18, false) == 73);
  CHECK(group_pos(18, true) == 72);
  CHECK(text_length(0, false) == 0 && text_length(54, false) == 73 && text_length(55, false) == 77);
  CHECK(text_length(54, true) == 72 && text_length(55, true) == 76 && text_length(2, true) == 4);
  CHECK(kEncMaxTextCap == 1451539875ull);
  CHECK(kEncUpdTileBytes == 6048 && kEncUpdTileText == 8176 && kEncUpdTileFlat == 8064);
}

static void test_refusals() {
  std::string why;
  Pairs p(4);
  const uint64_t off[3] = {0, 100, 200}, toff[3] = {0, 400, 800};
  const uint32_t size[3] = {100, 100, 56}, caps[3] = {400, 400, 100}, so[3] = {2, 0, 3};
  auto check = [&](const uint32_t* state_of, uint64_t data_len, const uint64_t* o, const uint32_t* sz, uint64_t n,
                   uint64_t text_len, const uint64_t* to, const uint32_t* cp) {
    return b64_encode_check(p.e.data(), p.s.data(), 4, state_of, data_len, o, sz, n, text_len, to, cp, why);
  };
  CHECK(check(so, 256, off, size, 3, 900, toff, caps) == kNoPiece);
  CHECK(check(nullptr, 256, off, size, 3, 900, toff, caps) == kNoPiece);
  // a piece outside [data, data + data_len); an empty piece may sit at the end
  CHECK(check(so, 255, off, size, 3, 900, toff, caps) == 2 && has(why, "outside [data"));
  const uint64_t far[1] = {UINT64_MAX}, at_end[1] = {256}, zero_off[1] = {0};
  const uint32_t one[1] = {1}, zero[1] = {0};
  CHECK(check(nullptr, 256, far, one, 1, 900, toff, caps) == 0 && has(why, "outside [data"));
  CHECK(check(nullptr, 256, at_end, zero, 1, 900, toff, caps) == kNoPiece);
  // a slot outside text; an empty slot may sit at the end
  CHECK(check(so, 256, off, size, 3, 899, toff, caps) == 2 && has(why, "slot outside"));
  CHECK(check(nullptr, 256, zero_off, one, 1, 900, far, one) == 0 && has(why, "slot outside"));
  const uint64_t text_end[1] = {900};
  CHECK(check(nullptr, 256, zero_off, one, 1, 900, text_end, zero) == kNoPiece);
  // a cap the launch would refuse, whatever text holds
  const uint32_t big[1] = {(uint32_t)b64e::kEncMaxTextCap + 1}, most[1] = {(uint32_t)b64e::kEncMaxTextCap};
  CHECK(check(nullptr, 256, zero_off, one, 1, 1ull << 40, zero_off, big) == 0 && has(why, "1 GiB"));
  CHECK(check(nullptr, 256, zero_off, one, 1, 1ull << 40, zero_off, most) == kNoPiece);
  // a state index >= n_states, named or implied
  const uint32_t so_bad[3] = {2, 4, 3};
  CHECK(check(so_bad, 256, off, size, 3, 900, toff, caps) == 1 && has(why, "state 4"));
  {
    std::string w2;
    CHECK(b64_encode_check(p.e.data(), p.s.data(), 2, nullptr, 256, off, size, 3, 900, toff, caps, w2) == 2);
    CHECK(has(w2, "state 2 of 2"));
  }
  // two pieces of one state: the later piece is named
  const uint32_t so_twice[3] = {2, 0, 2};
  CHECK(check(so_twice, 256, off, size, 3, 900, toff, caps) == 2 && has(why, "second piece of state 2"));
  // slots of different states that overlap; slots that touch, and empty ones inside another, are fine
  const uint64_t toff_over[3] = {0, 399, 800}, toff_touch[3] = {0, 400, 800};
  CHECK(check(so, 256, off, size, 3, 900, toff_over, caps) == 1 && has(why, "overlaps"));
  CHECK(check(so, 256, off, size, 3, 900, toff_touch, caps) == kNoPiece);
  const uint64_t toff_in[3] = {0, 400, 10};
  const uint32_t caps_in[3] = {400, 400, 0};
  CHECK(check(so, 256, off, size, 3, 900, toff_in, caps_in) == kNoPiece);
  // a chunk over 1 GiB: taken + size
  {
    Pairs q(1);
    q.at(0, (1ull << 30) - 50);
    const uint32_t s50[1] = {50}, s51[1] = {51};
    std::string w2;
    CHECK(b64_encode_check(q.e.data(), q.s.data(), 1, nullptr, 256, zero_off, s50, 1, 900, zero_off, one, w2) ==
          kNoPiece);
    CHECK(b64_encode_check(q.e.data(), q.s.data(), 1, nullptr, 256, zero_off, s51, 1, 900, zero_off, one, w2) == 0);
    CHECK(has(w2, "more than 1 GiB"));
  }
  // broken invariants of either record
  auto fault = [&](void (*spoil)(lbf_b64_enc_state&, lbf_sha1_state&), const char* what) {
    Pairs q(1);
    q.at(0, 100);
    CHECK(b64_enc_state_fault(q.e[0], q.s[0]).empty());
    spoil(q.e[0], q.s[0]);
    std::string w2;
    CHECK(b64_encode_check(q.e.data(), q.s.data(), 1, nullptr, 256, zero_off, one, 1, 900, zero_off, one, w2) == 0);
    CHECK(has(w2, "corrupt state") && has(w2, what));
  };
  fault([](lbf_b64_enc_state& e, lbf_sha1_state&) { e.ncarry = 2; }, "ncarry 2");
  fault([](lbf_b64_enc_state& e, lbf_sha1_state&) { e.ncarry = 3; }, "ncarry 3");
  fault([](lbf_b64_enc_state& e, lbf_sha1_state&) { e.carry = 0x100; }, "carry holds");
  fault([](lbf_b64_enc_state& e, lbf_sha1_state&) { e.layout = 2; }, "layout 2");
  fault([](lbf_b64_enc_state& e, lbf_sha1_state&) { e.zero = 1; }, "zero field");
  fault([](lbf_b64_enc_state& e, lbf_sha1_state& s) {
    e.taken = 1ull << 61;
    e.ncarry = (uint8_t)(e.taken % 3);
    e.carry = 0;
    s.total = e.taken;
    s.buffered = 0;
  }, "2^61");
  fault([](lbf_b64_enc_state&, lbf_sha1_state& s) { s.total = 99; s.buffered = 99 % 64; }, "is not taken 100");
  fault([](lbf_b64_enc_state&, lbf_sha1_state& s) { s.buffered = 64; }, "SHA state is corrupt");
  fault([](lbf_b64_enc_state&, lbf_sha1_state& s) { s.buffered = 5; }, "SHA state is corrupt");
}

// An oversized piece is cut where lbf_sha1_update_batch cuts it: update_plan.hpp's launches, multiples of 64.
static void test_oversized_piece_is_cut() {
  const uint64_t off[3] = {10, 5000, 9000};
  const uint32_t size[3] = {100, 3000, 50};
  const auto launches = update_launches(off, size, 3, 1024);
  // 100 | 896 of the big piece (what is left, down to a multiple of 64) ; 1024 ; 1024 ; 56 + the last piece
  CHECK(launches.size() == 4);
  CHECK(launches[0].size() == 2 && launches[0][1].piece == 1 && launches[0][1].size == 896 && !launches[0][1].last);
  CHECK(launches[1].size() == 1 && launches[1][0].off == 5000 + 896 && launches[1][0].size == 1024);
  CHECK(launches[2].size() == 1 && launches[2][0].size == 1024 && !launches[2][0].last);
  CHECK(launches[3].size() == 2 && launches[3][0].size == 56 && launches[3][0].last && launches[3][1].piece == 2);
  // the cuts' spans follow one another and end at the piece's text
  for (int flat = 0; flat < 2; ++flat) {
    uint64_t taken = 7, end = b64e::group_pos(7 / 3, flat != 0);
    for (uint32_t cut : {896u, 1024u, 1024u, 56u}) {
      const bool last = cut == 56;
      const B64EncSpan s = b64_encode_span(taken, cut, last, flat != 0, 1u << 20);
      CHECK(s.lo == end && s.hi >= s.lo);
      end = s.hi;
      taken += cut;
      if (last) CHECK(s.length == b64e::text_length(taken, flat != 0) && s.hi == s.length);
    }
    CHECK(taken == 3007);
  }
}

static void test_spans() {
  // 53 + 1 bytes: the second piece completes the line's 18th group and writes the separator behind it
  B64EncSpan s = b64_encode_span(0, 53, false, false, 1000);
  CHECK(s.lo == 0 && s.hi == 68);
  s = b64_encode_span(53, 1, false, false, 1000);
  CHECK(s.lo == 68 && s.hi == 73);
  s = b64_encode_span(53, 1, false, true, 1000);
  CHECK(s.lo == 68 && s.hi == 72);
  // a piece shorter than what completes the group writes nothing; a final one the last group
  s = b64_encode_span(4, 1, false, false, 1000);
  CHECK(s.lo == 4 && s.hi == 4);
  s = b64_encode_span(4, 1, true, false, 1000);
  CHECK(s.lo == 4 && s.hi == 8 && s.length == 8);
  s = b64_encode_span(4, 0, true, false, 1000);
  CHECK(s.lo == 4 && s.hi == 8 && s.length == 8);
  s = b64_encode_span(0, 0, true, false, 1000);
  CHECK(s.lo == 0 && s.hi == 0 && s.length == 0);
  // the cap clips both ends, and a text that does not fit reports cap + 1
  s = b64_encode_span(0, 167, true, false, 226);
  CHECK(s.lo == 0 && s.hi == 226 && s.length == 227);
  s = b64_encode_span(0, 167, true, false, 227);
  CHECK(s.hi == 227 && s.length == 227);
  s = b64_encode_span(300, 30, false, true, 100);
  CHECK(s.lo == 100 && s.hi == 100);
  s = b64_encode_span(0, 10, true, true, 0);
  CHECK(s.lo == 0 && s.hi == 0 && s.length == 1);
}

static void test_places_and_copyback() {
  std::vector<B64EncSpan> spans = {{0, 68, 0}, {73, 100, 0}, {5, 5, 0}, {1000, 1016, 0}, {16, 48, 0}};
  std::vector<B64EncPlace> places;
  const uint64_t area = b64_encode_places(spans, places);
  uint64_t cursor = 0;
  for (size_t k = 0; k < spans.size(); ++k) {
    CHECK(places[k].dev >= cursor && places[k].dev < cursor + 16);         // areas follow one another, no overlap
    CHECK(places[k].dev % 16 == spans[k].lo % 16);                         // at the text position's phase
    CHECK(places[k].room == spans[k].hi - spans[k].lo);
    CHECK(places[k].slot + spans[k].lo == places[k].dev);                  // mod 2^64
    cursor = places[k].dev + places[k].room;
  }
  CHECK(area == cursor);
  CHECK(places[0].dev == 0 && places[1].dev == 73 && places[3].slot == places[3].dev - 1000);
  // copy-back: ranges that touch on both sides travel as one run; empty ones vanish
  std::vector<uint64_t> dev = {0, 68, 200, 232, 300}, host = {1000, 1068, 5000, 5033, 7000};
  std::vector<uint32_t> size = {68, 5, 32, 10, 0};
  std::vector<Run> runs;
  copyback_runs(dev, host, size, runs);
  CHECK(runs.size() == 3);
  CHECK(runs[0].src == 0 && runs[0].dst == 1000 && runs[0].len == 73);
  CHECK(runs[1].src == 200 && runs[1].dst == 5000 && runs[1].len == 32);  // touches on the device only
  CHECK(runs[2].src == 232 && runs[2].dst == 5033 && runs[2].len == 10);
}

// Where an encode launch's tables lie: the numbers of the hand-written offset
// chain the layout replaced.  Encoder states (16 m) | SHA states (96 m) | piece
// offsets, slot starts, new offsets (8 m each) | piece sizes, caps, new
// lengths, text lengths (4 m each) | expected, digests (20 m each) | final
// flags, verdicts (m each).
static void test_table_offsets() {
  struct Want { uint64_t m, at[13]; };  // sha ... ver, bytes
  const Want want[3] = {{1, {16, 112, 120, 128, 136, 140, 144, 148, 152, 172, 192, 193, 194}},
                        {2, {32, 224, 240, 256, 272, 280, 288, 296, 304, 344, 384, 386, 388}},
                        {7, {112, 784, 840, 896, 952, 980, 1008, 1036, 1064, 1204, 1344, 1351, 1358}}};
  for (const Want& w : want) {
    const EncodeTables t = encode_tables(w.m);
    const uint64_t got[13] = {t.sha,  t.off,   t.slot, t.noff, t.size, t.cap, t.nlen,
                              t.tsize, t.exp,  t.dig,  t.fin,  t.ver,  t.bytes};
    CHECK(t.enc == 0);
    for (int k = 0; k < 13; ++k) CHECK(got[k] == w.at[k]);
  }
}

int main() {
  test_geometry();
  test_refusals();
  test_oversized_piece_is_cut();
  test_spans();
  test_places_and_copyback();
  test_table_offsets();
  if (g_fail) {
    std::printf("b64_encode_plan_tests: %d FAILED\n", g_fail);
    return 1;
  }
  std::printf("b64_encode_plan_tests: OK\n");
  return 0;
}
