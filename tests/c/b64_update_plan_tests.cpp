// b64_update_plan_tests.cpp -- the planner of lbf_b64_update_batch
// (bitflood_amd/csrc/b64_update_plan.hpp) on the CPU: every refusal, the bound
// on what a piece of text decodes to, where a launch's bytes lie on the device
// and how they come back.  Includes only that header and links nothing;
// tests/test_b64_update_cpu.py compiles it with plain g++ and again with
// -fsanitize=address,undefined and runs both.
#include "b64_update_plan.hpp"

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

struct Pairs {
  std::vector<lbf_b64_state> b;
  std::vector<lbf_sha1_state> s;
  explicit Pairs(size_t n) : b(n), s(n) {
    std::memset(b.data(), 0, n * sizeof(lbf_b64_state));
    std::memset(s.data(), 0, n * sizeof(lbf_sha1_state));
  }
  void at(size_t k, uint64_t decoded, uint64_t cap) {  // a consistent pair mid-chunk
    b[k].decoded = decoded;
    s[k].total = std::min(decoded, cap);
    s[k].buffered = (uint32_t)(s[k].total % 64);
  }
};

static bool has(const std::string& why, const char* what) { return why.find(what) != std::string::npos; }

static void test_refusals() {
  std::string why;
  Pairs p(4);
  const uint64_t toff[3] = {0, 100, 200}, ooff[3] = {0, 300, 600};
  const uint32_t tlen[3] = {100, 100, 56}, caps[3] = {300, 300, 100}, so[3] = {2, 0, 3};
  auto check = [&](const uint32_t* state_of, uint64_t text_len, const uint64_t* to, const uint32_t* tl, uint64_t n,
                   const uint32_t* cp, uint64_t out_len, const uint64_t* oo) {
    return b64_update_check(p.b.data(), p.s.data(), 4, state_of, text_len, to, tl, n, cp, out_len, oo, why);
  };
  CHECK(check(so, 256, toff, tlen, 3, caps, 700, ooff) == kNoPiece);
  CHECK(check(nullptr, 256, toff, tlen, 3, caps, 700, ooff) == kNoPiece);
  // text outside [text, text + text_len); an empty piece may sit at the end
  CHECK(check(so, 255, toff, tlen, 3, caps, 700, ooff) == 2 && has(why, "text outside"));
  const uint64_t far[1] = {UINT64_MAX}, at_end[1] = {256}, zero_off[1] = {0};
  const uint32_t one[1] = {1}, zero[1] = {0};
  CHECK(check(nullptr, 256, far, one, 1, caps, 700, ooff) == 0);
  CHECK(check(nullptr, 256, at_end, zero, 1, caps, 700, ooff) == kNoPiece);
  // a slot outside out; an empty slot may sit at the end
  CHECK(check(so, 256, toff, tlen, 3, caps, 699, ooff) == 2 && has(why, "slot outside"));
  CHECK(check(nullptr, 256, zero_off, one, 1, one, 700, far) == 0 && has(why, "slot outside"));
  const uint64_t out_end[1] = {700};
  CHECK(check(nullptr, 256, zero_off, one, 1, zero, 700, out_end) == kNoPiece);
  // a chunk over 1 GiB, whatever out holds
  const uint32_t big[1] = {(1u << 30) + 1}, gib[1] = {1u << 30};
  CHECK(check(nullptr, 256, zero_off, one, 1, big, 1ull << 40, zero_off) == 0 && has(why, "1 GiB"));
  CHECK(check(nullptr, 256, zero_off, one, 1, gib, 1ull << 40, zero_off) == kNoPiece);
  // a state index >= n_states, named or implied
  const uint32_t so_bad[3] = {2, 4, 3};
  CHECK(check(so_bad, 256, toff, tlen, 3, caps, 700, ooff) == 1 && has(why, "state 4"));
  {
    std::string w2;
    CHECK(b64_update_check(p.b.data(), p.s.data(), 2, nullptr, 256, toff, tlen, 3, caps, 700, ooff, w2) == 2);
  }
  // two pieces of one state: the later one is named
  const uint32_t so_dup[3] = {3, 0, 3};
  CHECK(check(so_dup, 256, toff, tlen, 3, caps, 700, ooff) == 2 && has(why, "second piece"));
  // slots of different states that overlap; touching is fine, and an empty slot overlaps nothing
  const uint64_t lap[3] = {0, 299, 600}, touch[3] = {0, 300, 599};
  CHECK(check(so, 256, toff, tlen, 3, caps, 700, lap) == 1 && has(why, "overlaps"));
  CHECK(check(so, 256, toff, tlen, 3, caps, 700, touch) == 2 && has(why, "overlaps"));
  const uint32_t caps0[3] = {300, 300, 0};
  CHECK(check(so, 256, toff, tlen, 3, caps0, 700, touch) == kNoPiece);
  // every invariant of the pair, one at a time (piece 1 continues state 0)
  auto refused = [&](const char* what) {
    const bool r = check(so, 256, toff, tlen, 3, caps, 700, ooff) == 1 && has(why, "corrupt") && has(why, what);
    p.b[0] = lbf_b64_state{};
    p.s[0] = lbf_sha1_state{};
    return r;
  };
  p.b[0].ncarry = 4;
  CHECK(refused("ncarry"));
  p.b[0].ncarry = 1;
  p.b[0].carry = 64;
  CHECK(refused("carry"));
  p.b[0].carry = 1;
  CHECK(refused("carry"));  // ncarry 0
  p.b[0].ended = 2;
  CHECK(refused("ended"));
  p.b[0].zero = 1;
  CHECK(refused("zero"));
  p.at(0, 4, 300);
  CHECK(refused("multiple of 3"));
  p.at(0, kUpdateMaxTotal, 300);
  p.b[0].ended = 1;
  CHECK(refused("2^61"));
  p.at(0, 6, 300);
  p.s[0].total = 3;
  p.s[0].buffered = 3;
  CHECK(refused("SHA state total"));
  p.at(0, 66, 300);
  p.s[0].buffered = 3;
  CHECK(refused("buffered"));
  // consistent pairs pass: mid-chunk, ended on any count, past the slot
  p.at(0, 66, 300);
  p.b[0].ncarry = 3;
  p.b[0].carry = (1u << 18) - 1;
  CHECK(check(so, 256, toff, tlen, 3, caps, 700, ooff) == kNoPiece);
  p.at(0, 67, 300);
  p.b[0].ended = 1;
  CHECK(check(so, 256, toff, tlen, 3, caps, 700, ooff) == kNoPiece);
  p.at(0, 3000, 300);
  CHECK(check(so, 256, toff, tlen, 3, caps, 700, ooff) == kNoPiece);
  // an untouched corrupt state does not matter
  p.b[1].ncarry = 9;
  CHECK(check(so, 256, toff, tlen, 3, caps, 700, ooff) == kNoPiece);
}

// The bound against the rule itself: every text of up to 7 characters over
// {sextet, '=', junk} after every carry.
static void test_bound() {
  for (uint32_t nc = 0; nc < 4; ++nc)
    for (uint32_t len = 0; len <= 7; ++len) {
      uint32_t combos = 1;
      for (uint32_t k = 0; k < len; ++k) combos *= 3;
      uint64_t most = 0;
      for (uint32_t code = 0; code < combos; ++code) {
        uint32_t pending = nc, x = code;
        uint64_t bytes = 0;
        for (uint32_t k = 0; k < len; ++k, x /= 3) {
          const uint32_t kind = x % 3;
          if (kind == 2) continue;  // junk
          if (kind == 1) {          // '='
            bytes += pending == 2 ? 1 : pending == 3 ? 2 : 0;
            break;
          }
          if (++pending == 4) {
            bytes += 3;
            pending = 0;
          }
        }
        most = std::max(most, bytes);
      }
      CHECK(most <= b64_decode_bound(nc, len));
      CHECK(b64_decode_bound(nc, len) <= most + 4);  // and it is no gross overestimate
    }
  CHECK(b64_decode_bound(3, UINT32_MAX) == 3 * ((3ull + UINT32_MAX) / 4) + 2);
}

static void test_places() {
  // chains at 0, mid-block, past a block, at the slot's end, past the slot
  const std::vector<uint64_t> decoded = {0, 57, 129, 300, 3000, 63, 0};
  const std::vector<uint32_t> ncarry = {0, 3, 1, 0, 2, 255, 0};
  const std::vector<uint32_t> len = {100, 8, 4096, 40, 40, 5, 0};
  const std::vector<uint32_t> cap = {300, 300, 1u << 20, 300, 300, 64, 0};
  std::vector<B64Place> pl;
  const uint64_t area = b64_update_places(decoded, ncarry, std::vector<uint64_t>(len.begin(), len.end()), cap, pl);
  uint64_t end = 0;
  for (size_t k = 0; k < pl.size(); ++k) {
    const uint64_t at = std::min<uint64_t>(decoded[k], cap[k]);
    CHECK(pl[k].dev >= end && pl[k].dev < end + 64);  // areas in order, moved up by less than a block
    CHECK(pl[k].dev % 64 == at % 64);                 // the update kernel's blocks start 64-byte aligned
    CHECK(pl[k].slot + at == pl[k].dev);              // mod 2^64
    CHECK(pl[k].room <= cap[k] - at);
    CHECK(pl[k].room <= b64_decode_bound(ncarry[k] & 3, len[k]));
    end = pl[k].dev + pl[k].room;
  }
  CHECK(area == end);
  CHECK(pl[0].room == 77 && pl[1].room == 3 * (11 / 4) + 2 && pl[3].room == 0 && pl[4].room == 0);
  CHECK(pl[5].room == 1);  // a forged ncarry counts & 3, and the slot has one byte left
  CHECK(pl[4].slot == pl[4].dev - 300);
  std::vector<B64Place> none;
  CHECK(b64_update_places({}, {}, {}, {}, none) == 0 && none.empty());
}

static void test_copyback() {
  std::vector<Run> runs;
  // touching on both sides joins; touching on one side only does not; empty pieces vanish
  copyback_runs({0, 10, 30, 64, 100}, {500, 510, 520, 900, 904}, {10, 10, 0, 4, 7}, runs);
  CHECK(runs.size() == 3);
  CHECK(runs[0].src == 0 && runs[0].dst == 500 && runs[0].len == 20);
  CHECK(runs[1].src == 64 && runs[1].dst == 900 && runs[1].len == 4);
  CHECK(runs[2].src == 100 && runs[2].dst == 904 && runs[2].len == 7);
  copyback_runs({0, 10}, {500, 511}, {10, 10}, runs);
  CHECK(runs.size() == 2);
  copyback_runs({}, {}, {}, runs);
  CHECK(runs.empty());
}

// Text is cut by update_launches: any cut is a legal stopping place of the
// decoder, the cuts of one piece are in order, one per launch, and only the
// last carries the final flag.
static void test_text_cutting() {
  const uint64_t offs[3] = {5, 5 + 300, 1000};
  const uint32_t lens[3] = {300, 0, 1000};
  const std::vector<std::vector<UpdateCut>> l = update_launches(offs, lens, 3, 256);
  uint64_t done[3] = {0, 0, 0};
  for (const auto& cuts : l) {
    uint64_t used = 0;
    bool seen[3] = {false, false, false};
    for (const UpdateCut& c : cuts) {
      CHECK(!seen[c.piece]);
      seen[c.piece] = true;
      CHECK(c.off == offs[c.piece] + done[c.piece]);
      done[c.piece] += c.size;
      CHECK(c.last == (done[c.piece] == lens[c.piece]));
      used += c.size;
    }
    CHECK(used <= 256);
  }
  CHECK(done[0] == 300 && done[1] == 0 && done[2] == 1000);
}

// Text and slots on both sides of byte 2^32 of the caller's buffers: pieces
// and slots that touch one another across the line, and one pair past 3 * 2^32.
static void test_past_4gib() {
  const uint64_t G = 1ull << 32;
  std::string why;
  Pairs p(4);
  const uint64_t toff[4] = {G - 70, G - 6, G + 64, 3 * G + 5};
  const uint32_t tlen[4] = {64, 70, 100, 33};
  const uint64_t ooff[4] = {G - 70, G - 6, G + 64, 3 * G + 5};
  const uint32_t caps[4] = {64, 70, 75, 24};  // the slots touch across the line too
  const uint64_t tend = 3 * G + 5 + 33, oend = 3 * G + 5 + 24;
  auto check = [&](uint64_t text_len, uint64_t out_len, uint64_t n, const uint64_t* oo = nullptr) {
    return b64_update_check(p.b.data(), p.s.data(), 4, nullptr, text_len, toff, tlen, n, caps, out_len, oo ? oo : ooff,
                            why);
  };
  // bounds exactly at, and one byte short of, the last piece's and the last slot's end
  CHECK(check(tend, oend, 4) == kNoPiece);
  CHECK(check(tend - 1, oend, 4) == 3 && has(why, "text outside"));
  CHECK(check(tend, oend - 1, 4) == 3 && has(why, "slot outside"));
  // buffers that end at the line, and just past the piece that straddles it
  CHECK(check(G, oend, 4) == 1 && has(why, "text outside"));
  CHECK(check(tend, G, 4) == 1 && has(why, "slot outside"));
  CHECK(check(G + 64, G + 64, 2) == kNoPiece);
  CHECK(check(G + 63, G + 64, 2) == 1 && check(G + 64, G + 63, 2) == 1);
  // lengths whose low 32 bits alone would do
  CHECK(check((uint32_t)tend + 2 * G, oend, 4) == 3 && check(tend, (uint32_t)oend + 2 * G, 4) == 3);
  // overlap is found across the line, touching is not
  const uint64_t lap[4] = {G - 70, G - 7, G + 64, 3 * G + 5};
  CHECK(check(tend, oend, 4, lap) == 1 && has(why, "overlaps"));
  const uint64_t wrapped[4] = {G - 70, G - 6, G + 64, G - 6 + 3 * G};  // equal to slot 1 mod 2^32 only
  CHECK(check(tend, 5 * G, 4, wrapped) == kNoPiece);

  // the text's cuts and their staging runs: joined across the line, phases kept
  const std::vector<std::vector<UpdateCut>> plan = update_launches(toff, tlen, 4, 1 << 20);
  CHECK(plan.size() == 1 && plan[0].size() == 4);
  std::vector<Run> runs;
  std::vector<uint64_t> dev;
  update_runs(plan[0], runs, dev);
  CHECK(runs.size() == 2);
  if (runs.size() == 2) {
    CHECK(runs[0].src == G - 70 && runs[0].len == 234 && runs[1].src == 3 * G + 5 && runs[1].len == 33);
    for (size_t k = 0; k < 4; ++k) CHECK(dev[k] % 16 == toff[k] % 16);
  }

  // places depend on chain positions alone, and the chains are past 2^32 as well
  const std::vector<uint64_t> decoded = {0, G + 3, 3 * G, 9};
  const std::vector<uint32_t> ncarry = {0, 1, 2, 3};
  const std::vector<uint32_t> len(tlen, tlen + 4), cap(caps, caps + 4);
  std::vector<B64Place> pl;
  const uint64_t area = b64_update_places(decoded, ncarry, std::vector<uint64_t>(len.begin(), len.end()), cap, pl);
  CHECK(area < 1024);
  for (size_t k = 0; k < 4; ++k) {
    const uint64_t at = std::min<uint64_t>(decoded[k], cap[k]);
    CHECK(pl[k].slot + at == pl[k].dev && pl[k].dev % 64 == at % 64 && pl[k].room <= cap[k] - at);
  }
  CHECK(pl[1].room == 0 && pl[2].room == 0 && pl[0].room == 50 && pl[3].room == 15);

  // copy-back: host positions are 64-bit; runs join across the line when both sides touch
  copyback_runs({0, 64, 140, 320}, {G - 70, G - 6, G + 64, 3 * G + 5}, {64, 70, 75, 24}, runs);
  CHECK(runs.size() == 3);
  if (runs.size() == 3) {
    CHECK(runs[0].src == 0 && runs[0].dst == G - 70 && runs[0].len == 134);  // across the line in one run
    CHECK(runs[1].src == 140 && runs[1].dst == G + 64 && runs[1].len == 75);  // host side touches, device side does not
    CHECK(runs[2].src == 320 && runs[2].dst == 3 * G + 5 && runs[2].len == 24);
  }
  copyback_runs({0, 64}, {G - 64, 2 * G}, {64, 10}, runs);  // host positions equal mod 2^32 do not touch
  CHECK(runs.size() == 2 && runs[1].dst == 2 * G);
}

// The one-piece and the seq checker over seeded calls (check_cases.hpp): each
// answers what tests/golden/plan_checks.txt records of the checkers before the
// planners were merged, and where no state repeats the two agree to the word.
static void test_checkers_agree() {
  using namespace plan_cases;
  const std::vector<Recorded> want = read_fixture(fixture_path(__FILE__));
  CHECK(want.size() == kCases);
  if (want.size() != kCases) return;
  uint64_t refused = 0;
  for (uint64_t k = 0; k < kCases; ++k) {
    const Case c = make_case(k);
    CHECK(checksum(c) == want[k].sum);
    Answer one, seq;
    one.piece = b64_update_check(c.b64.data(), c.sha.data(), c.n_states, c.so(), c.text_len, c.text_offsets.data(),
                                 c.text_lens.data(), c.n, c.caps.data(), c.out_len, c.out_offsets.data(), one.why);
    seq.piece = b64_update_seq_check(c.b64.data(), c.sha.data(), c.n_states, c.so(), c.text_len,
                                     c.text_offsets.data(), c.text_lens.data(), nullptr, c.n, c.caps.data(), c.out_len,
                                     c.out_offsets.data(), seq.why);
    CHECK(one == want[k].text_one);
    CHECK(seq == want[k].text_seq);
    if (!c.repeats) CHECK(one == seq);
    refused += one.piece != kNoPiece;
  }
  CHECK(refused > kCases / 4);
}

// Where a text launch's tables lie: the numbers of the hand-written offset
// chains the layout replaced.  b64 states (16 nc) | SHA states (96 nc) | text
// offsets, slot starts, piece offsets (8 m each) | seq only: chain_first
// (4 (nc + 1)) | text lengths, chunk sizes, piece sizes, decoded lengths, line
// and flat characters (4 m each) | expected, digests (20 m each) | final flags,
// verdicts (m each).
static void test_table_offsets() {
  struct Want { uint64_t m, nc; bool seq; uint64_t at[16]; };  // sha ... ver, bytes, in the order above
  const Want want[8] = {
      {1, 1, false, {16, 112, 120, 128, 136, 136, 140, 144, 148, 152, 156, 160, 180, 200, 201, 202}},
      {2, 2, false, {32, 224, 240, 256, 272, 272, 280, 288, 296, 304, 312, 320, 360, 400, 402, 404}},
      {7, 7, false, {112, 784, 840, 896, 952, 952, 980, 1008, 1036, 1064, 1092, 1120, 1260, 1400, 1407, 1414}},
      {1, 1, true, {16, 112, 120, 128, 136, 144, 148, 152, 156, 160, 164, 168, 188, 208, 209, 210}},
      {2, 1, true, {16, 112, 128, 144, 160, 168, 176, 184, 192, 200, 208, 216, 256, 296, 298, 300}},
      {2, 2, true, {32, 224, 240, 256, 272, 284, 292, 300, 308, 316, 324, 332, 372, 412, 414, 416}},
      {7, 1, true, {16, 112, 168, 224, 280, 288, 316, 344, 372, 400, 428, 456, 596, 736, 743, 750}},
      {7, 7, true, {112, 784, 840, 896, 952, 984, 1012, 1040, 1068, 1096, 1124, 1152, 1292, 1432, 1439, 1446}}};
  for (const Want& w : want) {
    const TextTables t = text_tables(w.m, w.nc, w.seq);
    const uint64_t got[16] = {t.sha,   t.toff,  t.slot,  t.poff, t.first, t.tlen, t.cap, t.psize,
                              t.osize, t.lines, t.flat,  t.exp,  t.dig,   t.fin,  t.ver, t.bytes};
    CHECK(t.b64 == 0);
    for (int k = 0; k < 16; ++k) CHECK(got[k] == w.at[k]);
  }
}

int main() {
  test_refusals();
  test_bound();
  test_places();
  test_copyback();
  test_text_cutting();
  test_past_4gib();
  test_checkers_agree();
  test_table_offsets();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("b64_update_plan_tests: OK\n");
  return 0;
}
