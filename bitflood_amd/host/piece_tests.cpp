// piece_tests.cpp -- libBitFlood::PieceHasher on the GPU (run by
// tests/test_gpu_update.py): 64 chunks of 0..70,000 bytes hashed piece by
// piece, every string equal to Encoder::Base64Encode of the whole chunk;
// BytesIn, Reset, and a slot reused after its last piece.
//   lbf_piece_tests
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "libBitFlood/Encoder.H"
#include "libBitFlood/PieceHasher.H"

using namespace libBitFlood;

static int g_fail = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #cond);   \
      ++g_fail;                                                                      \
    }                                                                                \
  } while (0)

static U32 g_x = 0x9E3779B9u;
static U32 rnd() {
  g_x ^= g_x << 13;
  g_x ^= g_x >> 17;
  g_x ^= g_x << 5;
  return g_x;
}

int main() {
  const U32 kSlots = 64;
  // chunk c lives at start[c] of one arena; sizes cover 0, 1, the block edges and ragged lengths up to 70,000
  std::vector<U32> size(kSlots);
  const U32 edges[] = {0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 70000};
  for (U32 c = 0; c < kSlots; ++c) size[c] = c < sizeof edges / sizeof *edges ? edges[c] : rnd() % 70001;
  std::vector<U64> start(kSlots);
  U64 len = 0;
  for (U32 c = 0; c < kSlots; ++c) {
    start[c] = len;
    len += size[c] + (rnd() % 3);  // chunks at every alignment
  }
  std::vector<U8> arena(len + 1);
  for (U8& b : arena) b = (U8)(rnd() >> 24);

  std::vector<std::string> want(kSlots);
  for (U32 c = 0; c < kSlots; ++c)
    if (Encoder::Base64Encode(arena.data() + start[c], size[c], want[c]) != Error::NO_ERROR_LBF) {
      std::fprintf(stderr, "no GPU path: %s\n", Encoder::LastError());
      return 1;
    }

  PieceHasher ph(kSlots);
  CHECK(ph.Slots() == kSlots);
  std::vector<U32> done(kSlots, 0);
  std::vector<std::string> got(kSlots);
  std::vector<bool> finished(kSlots, false);
  // rounds of one piece per unfinished chunk, pieces of 0..20,000 bytes
  for (int round = 0; round < 64; ++round) {
    PieceHasher::V_Piece pieces;
    for (U32 c = 0; c < kSlots; ++c) {
      if (finished[c]) continue;
      PieceHasher::Piece p;
      p.m_slot = c;
      p.m_offset = start[c] + done[c];
      p.m_size = std::min<U32>(size[c] - done[c], rnd() % 20001);
      p.m_last = done[c] + p.m_size == size[c] && ((rnd() & 1) || round > 40);  // sometimes a later, empty last piece
      pieces.push_back(p);
    }
    if (pieces.empty()) break;
    V_String hashes;
    CHECK(ph.Update(arena.data(), arena.size(), pieces, hashes) == Error::NO_ERROR_LBF);
    CHECK(hashes.size() == pieces.size());
    for (size_t k = 0; k < pieces.size() && k < hashes.size(); ++k) {
      const U32 c = pieces[k].m_slot;
      done[c] += pieces[k].m_size;
      if (pieces[k].m_last) {
        CHECK(hashes[k].size() == 27 && hashes[k] == want[c]);
        CHECK(ph.BytesIn(c) == 0);  // Final() restarts the slot
        finished[c] = true;
        got[c] = hashes[k];
      } else {
        CHECK(hashes[k].empty());
        CHECK(ph.BytesIn(c) == done[c]);
      }
    }
  }
  for (U32 c = 0; c < kSlots; ++c) CHECK(finished[c] && got[c] == want[c]);

  // a slot reused after its last piece, and Reset dropping an unfinished chunk
  {
    V_String hashes;
    PieceHasher::V_Piece one(1);
    one[0].m_slot = 10;
    one[0].m_offset = start[10];
    one[0].m_size = size[10] / 2;
    CHECK(ph.Update(arena.data(), arena.size(), one, hashes) == Error::NO_ERROR_LBF);
    CHECK(ph.BytesIn(10) == size[10] / 2);
    ph.Reset(10);
    CHECK(ph.BytesIn(10) == 0);
    one[0].m_size = size[10];
    one[0].m_last = true;
    CHECK(ph.Update(arena.data(), arena.size(), one, hashes) == Error::NO_ERROR_LBF);
    CHECK(hashes.size() == 1 && hashes[0] == want[10]);
    CHECK(ph.BytesIn(kSlots) == 0);
    // refused: two pieces of one slot, a slot that does not exist, a piece outside the arena
    PieceHasher::V_Piece two(2);
    two[0].m_slot = two[1].m_slot = 3;
    CHECK(ph.Update(arena.data(), arena.size(), two, hashes) == Error::UNKNOWN_ERROR_LBF);
    two[1].m_slot = kSlots;
    CHECK(ph.Update(arena.data(), arena.size(), two, hashes) == Error::UNKNOWN_ERROR_LBF);
    two[1].m_slot = 4;
    two[1].m_offset = arena.size();
    two[1].m_size = 1;
    CHECK(ph.Update(arena.data(), arena.size(), two, hashes) == Error::UNKNOWN_ERROR_LBF);
    CHECK(ph.BytesIn(3) == 0 && ph.BytesIn(4) == 0);
  }

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("piece_tests OK\n");
  return 0;
}
