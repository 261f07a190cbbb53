// seq_piece_tests.cpp -- libBitFlood::PieceHasher::UpdateSeq and UpdateTextSeq on
// the GPU (run by tests/test_gpu_piece_seq.py): three slots with several pieces
// each in one call, interleaved, against the hash strings recorded in
// tests/golden/kat.json ("abc", the 56-byte NIST message, 64 KiB of zeros) --
// first as bytes, then as xmlrpc++ text whose pieces split groups; then a chunk
// spread over two calls, what the calls refuse, and that Update / UpdateText
// still refuse two pieces of one slot.
//   lbf_seq_piece_tests
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "libBitFlood/PeerWire.H"
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

// Cut [0, len) at `cuts` places spread by a small generator; the cuts are
// sorted, may repeat (empty pieces) and include 0 and len as ends.
static std::vector<U32> cut_points(U32 len, U32 cuts, U32 seed) {
  std::vector<U32> at = {0, len};
  U32 x = seed * 2654435761u + 12345u;
  for (U32 k = 0; k < cuts; ++k) {
    x = x * 1664525u + 1013904223u;
    at.push_back(len ? (x >> 8) % (len + 1) : 0);
  }
  std::sort(at.begin(), at.end());
  return at;
}

int main() {
  // tests/golden/kat.json: abc, nist448, zeros_64KiB
  const std::string nist = "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq";
  const std::vector<std::string> want = {"qZk+NkcGgWq6PiVxeFDCbJzQ2J0", "hJg+RBw70m66rkqh+VEp5eVGcPE",
                                         "GtyVvr6e6owRLUDNBKt6jXXE+WE"};
  std::vector<std::vector<U8>> chunk(3);
  chunk[0].assign({'a', 'b', 'c'});
  chunk[1].assign(nist.begin(), nist.end());
  chunk[2].assign(65536, 0);
  const U32 kSlots = 3, kGuard = 7;
  const U32 ncuts[3] = {2, 5, 6};  // slot c goes as ncuts[c] + 1 pieces

  // ---- bytes: the chunks follow one another in the arena, every piece of every slot in ONE call
  {
    std::vector<U8> arena;
    std::vector<U64> start(kSlots);
    for (U32 c = 0; c < kSlots; ++c) {
      start[c] = arena.size();
      arena.insert(arena.end(), chunk[c].begin(), chunk[c].end());
    }
    std::vector<std::vector<U32>> at(kSlots);
    for (U32 c = 0; c < kSlots; ++c) at[c] = cut_points((U32)chunk[c].size(), ncuts[c], 7 + c);
    PieceHasher::V_Piece pieces;
    for (U32 round = 0; round < 8; ++round)  // interleaved: piece `round` of each slot that has one
      for (U32 k = 0; k < kSlots; ++k) {
        const U32 c = (k + round) % kSlots;
        if (round + 1 >= at[c].size()) continue;
        PieceHasher::Piece p;
        p.m_slot = c;
        p.m_offset = start[c] + at[c][round];
        p.m_size = at[c][round + 1] - at[c][round];
        p.m_last = round + 2 == at[c].size();
        pieces.push_back(p);
      }
    PieceHasher ph(kSlots);
    V_String hashes;
    CHECK(ph.Update(arena.data(), arena.size(), pieces, hashes) == Error::UNKNOWN_ERROR_LBF);  // one piece per slot
    for (U32 c = 0; c < kSlots; ++c) CHECK(ph.BytesIn(c) == 0);
    CHECK(ph.UpdateSeq(arena.data(), arena.size(), pieces, hashes) == Error::NO_ERROR_LBF);
    CHECK(hashes.size() == pieces.size());
    for (size_t k = 0; k < pieces.size() && k < hashes.size(); ++k)
      CHECK(hashes[k] == (pieces[k].m_last ? want[pieces[k].m_slot] : std::string()));
    for (U32 c = 0; c < kSlots; ++c) CHECK(ph.BytesIn(c) == 0);  // every chunk is over

    // a chunk over two calls, two pieces of it in each; the other slots idle
    PieceHasher::V_Piece half(2);
    half[0].m_slot = half[1].m_slot = 1;
    half[0].m_offset = start[1];
    half[0].m_size = 5;
    half[1].m_offset = start[1] + 5;
    half[1].m_size = 20;
    CHECK(ph.UpdateSeq(arena.data(), arena.size(), half, hashes) == Error::NO_ERROR_LBF);
    CHECK(ph.BytesIn(1) == 25 && hashes[0].empty() && hashes[1].empty());
    half[0].m_offset = start[1] + 25;
    half[0].m_size = 0;
    half[1].m_offset = start[1] + 25;
    half[1].m_size = 31;
    half[1].m_last = true;
    CHECK(ph.UpdateSeq(arena.data(), arena.size(), half, hashes) == Error::NO_ERROR_LBF);
    CHECK(hashes[0].empty() && hashes[1] == want[1] && ph.BytesIn(1) == 0);

    // refused, states untouched: a last piece that another piece of its slot follows; no such slot; bytes outside
    half[0].m_last = true;
    CHECK(ph.UpdateSeq(arena.data(), arena.size(), half, hashes) == Error::UNKNOWN_ERROR_LBF);
    half[0].m_last = false;
    half[1].m_slot = kSlots;
    CHECK(ph.UpdateSeq(arena.data(), arena.size(), half, hashes) == Error::UNKNOWN_ERROR_LBF);
    half[1].m_slot = 1;
    half[1].m_offset = arena.size();
    half[1].m_size = 1;
    CHECK(ph.UpdateSeq(arena.data(), arena.size(), half, hashes) == Error::UNKNOWN_ERROR_LBF);
    CHECK(ph.BytesIn(1) == 0);
  }

  // ---- text: the texts follow one another, the slots lie in the arena with guard bytes around each
  {
    std::string text;
    std::vector<U64> tstart(kSlots), ostart(kSlots);
    std::vector<U32> tlen(kSlots);
    U64 alen = kGuard;
    for (U32 c = 0; c < kSlots; ++c) {
      tstart[c] = text.size();
      PeerWire::Base64Put(chunk[c].data(), chunk[c].size(), text);
      tlen[c] = (U32)(text.size() - tstart[c]);
      ostart[c] = alen;
      alen += chunk[c].size() + kGuard;
    }
    std::vector<U8> arena(alen, 0xEE), expect(alen, 0xEE);
    for (U32 c = 0; c < kSlots; ++c) std::copy(chunk[c].begin(), chunk[c].end(), expect.begin() + ostart[c]);
    std::vector<std::vector<U32>> at(kSlots);
    for (U32 c = 0; c < kSlots; ++c) at[c] = cut_points(tlen[c], ncuts[c], 31 + c);
    // two calls: the first takes the first two pieces of every slot, the second the rest
    PieceHasher ph(kSlots);
    for (int call = 0; call < 2; ++call) {
      PieceHasher::V_TextPiece pieces;
      V_String expected;
      for (U32 round = call ? 2 : 0; round < (call ? 8u : 2u); ++round)
        for (U32 k = 0; k < kSlots; ++k) {
          const U32 c = (k + round) % kSlots;
          if (round + 1 >= at[c].size()) continue;
          PieceHasher::TextPiece p;
          p.m_slot = c;
          p.m_text_offset = tstart[c] + at[c][round];
          p.m_text_len = at[c][round + 1] - at[c][round];
          p.m_out_offset = ostart[c];
          p.m_chunk_size = (U32)chunk[c].size();
          p.m_last = round + 2 == at[c].size();
          pieces.push_back(p);
          expected.push_back(p.m_last ? want[c] : std::string());
        }
      std::vector<U8> verdicts;
      std::vector<U32> sizes;
      if (call == 0)  // UpdateText still takes one piece per slot
        CHECK(ph.UpdateText(text.data(), text.size(), pieces, arena.data(), arena.size(), expected, verdicts, &sizes) ==
              Error::UNKNOWN_ERROR_LBF);
      CHECK(ph.UpdateTextSeq(text.data(), text.size(), pieces, arena.data(), arena.size(), expected, verdicts,
                             &sizes) == Error::NO_ERROR_LBF);
      CHECK(verdicts.size() == pieces.size() && sizes.size() == pieces.size());
      for (size_t k = 0; k < pieces.size() && k < verdicts.size(); ++k) {
        const U32 c = pieces[k].m_slot;
        if (pieces[k].m_last) {
          CHECK(verdicts[k] == 1 && sizes[k] == chunk[c].size());
        } else {
          CHECK(verdicts[k] == 0 && sizes[k] == 0);
        }
      }
      if (call == 0)
        for (U32 c = 0; c < kSlots; ++c) CHECK(ph.BytesIn(c) <= chunk[c].size());
    }
    for (U32 c = 0; c < kSlots; ++c) CHECK(ph.BytesIn(c) == 0);
    CHECK(arena == expect);  // the chunks where they belong, every guard byte as it was

    // refused, states and arena untouched: pieces of one slot that name different slots of the arena or chunk
    // sizes; a last piece that another piece of its slot follows
    std::vector<U8> verdicts;
    const V_String none(2);
    PieceHasher::V_TextPiece two(2);
    two[0].m_slot = two[1].m_slot = 1;
    two[0].m_text_offset = two[1].m_text_offset = tstart[1];
    two[0].m_text_len = two[1].m_text_len = 4;
    two[0].m_out_offset = ostart[1];
    two[1].m_out_offset = ostart[1] + 1;
    two[0].m_chunk_size = two[1].m_chunk_size = 56;
    CHECK(ph.UpdateTextSeq(text.data(), text.size(), two, arena.data(), arena.size(), none, verdicts, nullptr) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_out_offset = ostart[1];
    two[1].m_chunk_size = 55;
    CHECK(ph.UpdateTextSeq(text.data(), text.size(), two, arena.data(), arena.size(), none, verdicts, nullptr) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_chunk_size = 56;
    two[0].m_last = true;
    CHECK(ph.UpdateTextSeq(text.data(), text.size(), two, arena.data(), arena.size(), {want[1], std::string()},
                           verdicts, nullptr) == Error::UNKNOWN_ERROR_LBF);
    CHECK(ph.BytesIn(1) == 0);
    CHECK(arena == expect);
  }

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("seq_piece_tests OK\n");
  return 0;
}
