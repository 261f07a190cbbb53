// check_cases.hpp -- seeded calls for the planners' refusal rules, and the
// reader of tests/golden/plan_checks.txt, which records what the one-piece and
// the seq checkers answered to each of them before the planners were merged
// (update_plan_tests.cpp takes the hash half, b64_update_plan_tests.cpp the text
// half).  The generator draws from its own splitmix64, so a case is the same
// numbers on every machine; the fixture carries a checksum of each case's
// inputs, so a generator that drifted fails loudly instead of comparing other
// calls.  No final flags: where no state repeats, the one-piece and the seq
// checker must then agree to the piece and the word.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <vector>

#include "lbf_hash.h"

namespace plan_cases {

constexpr uint64_t kCases = 600;
constexpr uint64_t kTwo61 = 1ull << 61;

struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return next() % n; }
  bool one_in(uint64_t n) { return below(n) == 0; }
};

struct Case {
  uint64_t n = 0, n_states = 0;
  bool has_state_of = false, repeats = false;
  std::vector<uint32_t> state_of;
  // hash call
  uint64_t base_len = 0;
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> sizes;
  std::vector<lbf_sha1_state> states;
  // text call
  uint64_t text_len = 0, out_len = 0;
  std::vector<uint64_t> text_offsets, out_offsets;
  std::vector<uint32_t> text_lens, caps;
  std::vector<lbf_b64_state> b64;
  std::vector<lbf_sha1_state> sha;
  const uint32_t* so() const { return has_state_of ? state_of.data() : nullptr; }
};

inline void set_total(lbf_sha1_state& s, uint64_t total) {
  s.total = total;
  s.buffered = (uint32_t)(total % 64);
}

inline Case make_case(uint64_t idx) {
  Rng r{0xB17F100Dull * (idx + 1)};
  Case c;
  c.n_states = 1 + r.below(12);
  const bool want_repeats = idx % 5 < 2;
  c.n = want_repeats ? 1 + r.below(12) : 1 + r.below(c.n_states);
  c.has_state_of = want_repeats || !r.one_in(4);
  std::vector<uint32_t> perm(c.n_states);
  for (uint64_t k = 0; k < c.n_states; ++k) perm[k] = (uint32_t)k;
  for (uint64_t k = c.n_states; k > 1; --k) std::swap(perm[k - 1], perm[r.below(k)]);
  c.state_of.resize(c.n);
  for (uint64_t i = 0; i < c.n; ++i)
    c.state_of[i] = want_repeats ? (uint32_t)r.below(c.n_states) : c.has_state_of ? perm[i] : (uint32_t)i;
  if (c.has_state_of && r.one_in(10)) c.state_of[r.below(c.n)] = (uint32_t)(c.n_states + r.below(3));
  for (uint64_t i = 0; i < c.n; ++i)
    for (uint64_t j = 0; j < i; ++j) c.repeats |= c.state_of[i] == c.state_of[j];

  // the hash call: pieces of 0..96 bytes in a source of 4096
  c.base_len = 4096;
  c.offsets.resize(c.n);
  c.sizes.resize(c.n);
  for (uint64_t i = 0; i < c.n; ++i) {
    c.offsets[i] = r.below(4000);
    c.sizes[i] = (uint32_t)r.below(97);
  }
  if (r.one_in(8)) {
    const uint64_t i = r.below(c.n);
    c.offsets[i] = r.one_in(2) ? UINT64_MAX - r.below(4) : c.base_len - 5;
    c.sizes[i] = 6 + (uint32_t)r.below(10);
  }
  c.states.resize(c.n_states);
  for (lbf_sha1_state& s : c.states) {
    s = lbf_sha1_state{};
    set_total(s, r.below(100000));
  }
  if (r.one_in(5)) {  // a chain that stands near 2^61: a piece, or the sum of several, takes it past
    lbf_sha1_state& s = c.states[r.below(c.n_states)];
    set_total(s, r.one_in(6) ? kTwo61 + 1 + r.below(64) : kTwo61 - r.below(200));
  }
  if (r.one_in(6)) {
    lbf_sha1_state& s = c.states[r.below(c.n_states)];
    if (r.one_in(2))
      s.buffered = 64 + (uint32_t)r.below(5);
    else
      s.buffered = (s.buffered + 1 + (uint32_t)r.below(62)) % 64;
  }

  // the text call: a slot per piece, one behind the other with gaps; pieces of one state share nothing here
  c.text_len = 4096;
  c.text_offsets.resize(c.n);
  c.text_lens.resize(c.n);
  c.caps.resize(c.n);
  c.out_offsets.resize(c.n);
  uint64_t cursor = r.below(8);
  for (uint64_t i = 0; i < c.n; ++i) {
    c.text_offsets[i] = r.below(4000);
    c.text_lens[i] = (uint32_t)r.below(97);
    c.caps[i] = r.one_in(7) ? 0 : (uint32_t)r.below(300);
    c.out_offsets[i] = cursor;
    cursor += c.caps[i] + (r.one_in(3) ? 0 : r.below(5));
  }
  c.out_len = cursor;
  if (r.one_in(8)) {
    const uint64_t i = r.below(c.n);
    c.text_offsets[i] = c.text_len - 3;
    c.text_lens[i] = 4 + (uint32_t)r.below(4);
  }
  if (c.n > 1 && r.one_in(6)) {  // slots that overlap (or, of empty slots, do not)
    const uint64_t i = r.below(c.n), j = r.below(c.n);
    if (i != j) c.out_offsets[i] = c.out_offsets[j] + r.below(3);
  }
  if (r.one_in(10)) c.out_len -= std::min<uint64_t>(c.out_len, 1 + r.below(4));
  if (r.one_in(12)) c.caps[r.below(c.n)] = (1u << 30) + 1 + (uint32_t)r.below(9);
  c.b64.resize(c.n_states);
  c.sha.resize(c.n_states);
  for (uint64_t s = 0; s < c.n_states; ++s) {
    c.b64[s] = lbf_b64_state{};
    c.sha[s] = lbf_sha1_state{};
  }
  for (uint64_t i = 0; i < c.n; ++i) {  // each touched pair stands somewhere in (or past) its piece's chunk
    const uint64_t s = c.state_of[i];
    if (s >= c.n_states) continue;
    const uint64_t cap = c.caps[i];
    lbf_b64_state& b = c.b64[s];
    b.decoded = 3 * r.below(cap / 3 + 2);
    b.ncarry = (uint8_t)r.below(4);
    b.carry = (uint32_t)r.below(1ull << (6 * b.ncarry));
    set_total(c.sha[s], std::min<uint64_t>(b.decoded, cap));
  }
  if (r.one_in(4)) {
    const uint64_t s = r.below(c.n_states);
    lbf_b64_state& b = c.b64[s];
    switch (r.below(8)) {
      case 0: b.ncarry = 4; break;
      case 1: b.carry = 1u << (6 * (b.ncarry & 3u)); break;
      case 2: b.ended = 2; break;
      case 3: b.zero = 1; break;
      case 4: b.decoded += 1; break;
      case 5: b.decoded = kTwo61 + 3 * r.below(3); break;
      case 6: c.sha[s].buffered = 64; break;
      default: set_total(c.sha[s], c.sha[s].total + 1); break;
    }
  }
  return c;
}

inline uint64_t fnv(uint64_t h, const void* p, size_t bytes) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 0x100000001B3ull;
  return h;
}

template <class T>
uint64_t fnv_vec(uint64_t h, const std::vector<T>& v) {
  return v.empty() ? h : fnv(h, v.data(), v.size() * sizeof(T));
}

inline uint64_t checksum(const Case& c) {
  uint64_t h = 0xCBF29CE484222325ull;
  const uint64_t head[6] = {c.n, c.n_states, c.has_state_of, c.base_len, c.text_len, c.out_len};
  h = fnv(h, head, sizeof head);
  h = fnv_vec(h, c.state_of);
  h = fnv_vec(h, c.offsets);
  h = fnv_vec(h, c.sizes);
  h = fnv_vec(h, c.states);
  h = fnv_vec(h, c.text_offsets);
  h = fnv_vec(h, c.text_lens);
  h = fnv_vec(h, c.caps);
  h = fnv_vec(h, c.out_offsets);
  h = fnv_vec(h, c.b64);
  return fnv_vec(h, c.sha);
}

// One checker's answer: the piece it names (UINT64_MAX for none) and its words.
struct Answer {
  uint64_t piece = UINT64_MAX;
  std::string why;
  bool operator==(const Answer& o) const { return piece == o.piece && why == o.why; }
};

// What the fixture records of one case: the one-piece and the seq checker, for hash and for text.
struct Recorded {
  uint64_t sum = 0;
  Answer hash_one, hash_seq, text_one, text_seq;
};

inline std::string fixture_path(const char* this_file) {
  const std::string f(this_file);
  const size_t cut = f.find_last_of('/');
  return (cut == std::string::npos ? std::string(".") : f.substr(0, cut)) + "/../golden/plan_checks.txt";
}

// The fixture: per case a line "case <idx> <checksum>" and four lines "<piece or -> <why>".
inline std::vector<Recorded> read_fixture(const std::string& path) {
  std::vector<Recorded> all;
  std::ifstream in(path);
  std::string word;
  uint64_t idx = 0;
  while (in >> word >> idx) {
    if (word != "case" || idx != all.size()) return {};
    Recorded rec;
    in >> rec.sum;
    in.ignore(1, '\n');
    for (Answer* a : {&rec.hash_one, &rec.hash_seq, &rec.text_one, &rec.text_seq}) {
      std::string line;
      if (!std::getline(in, line)) return {};
      const size_t sp = line.find(' ');
      const std::string piece = line.substr(0, sp);
      a->piece = piece == "-" ? UINT64_MAX : std::stoull(piece);
      a->why = sp == std::string::npos ? std::string() : line.substr(sp + 1);
    }
    all.push_back(rec);
  }
  return all;
}

}  // namespace plan_cases
