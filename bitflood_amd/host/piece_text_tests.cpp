// piece_text_tests.cpp -- libBitFlood::PieceHasher fed base64 text on the GPU
// (run by tests/test_gpu_b64_update.py): three chunks whose hash strings are
// recorded in tests/golden/kat.json ("abc", the 56-byte NIST message, 64 KiB
// of zeros) arrive as xmlrpc++ text, cut into interleaved pieces at places
// that split groups; the arena receives exactly the chunks' bytes; then
// BytesIn, Reset, a text that decodes to too much, and the refusals.
//   lbf_piece_text_tests
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
  // the texts follow one another, the slots lie in the arena with guard bytes around each
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
  std::vector<U8> arena(alen, 0xEE);

  PieceHasher ph(kSlots);
  // rounds of interleaved pieces: slot c takes step[c] characters a round (odd steps split groups)
  const U32 step[3] = {1, 7, 30001};
  std::vector<U32> done(kSlots, 0);
  std::vector<bool> finished(kSlots, false);
  for (int round = 0; round < 16; ++round) {
    PieceHasher::V_TextPiece pieces;
    V_String expected;
    for (U32 k = 0; k < kSlots; ++k) {
      const U32 c = (k + round) % kSlots;  // the order of the slots changes from call to call
      if (finished[c]) continue;
      PieceHasher::TextPiece p;
      p.m_slot = c;
      p.m_text_offset = tstart[c] + done[c];
      p.m_text_len = std::min<U32>(step[c], tlen[c] - done[c]);
      p.m_out_offset = ostart[c];
      p.m_chunk_size = (U32)chunk[c].size();
      // slot 0's last piece is empty: the flag comes alone, after the text
      p.m_last = c == 0 ? done[c] == tlen[c] : done[c] + p.m_text_len == tlen[c];
      pieces.push_back(p);
      expected.push_back(p.m_last ? want[c] : std::string());
    }
    if (pieces.empty()) break;
    std::vector<U8> verdicts;
    std::vector<U32> sizes;
    CHECK(ph.UpdateText(text.data(), text.size(), pieces, arena.data(), arena.size(), expected, verdicts, &sizes) ==
          Error::NO_ERROR_LBF);
    CHECK(verdicts.size() == pieces.size() && sizes.size() == pieces.size());
    for (size_t k = 0; k < pieces.size() && k < verdicts.size(); ++k) {
      const U32 c = pieces[k].m_slot;
      done[c] += pieces[k].m_text_len;
      if (pieces[k].m_last) {
        CHECK(verdicts[k] == 1 && sizes[k] == chunk[c].size());
        CHECK(ph.BytesIn(c) == 0);  // the chunk is over: the slot starts its next one
        finished[c] = true;
      } else {
        CHECK(verdicts[k] == 0 && sizes[k] == 0);
        // every complete group so far, counted without the separators
        U64 sextets = 0;
        for (U32 j = 0; j < done[c]; ++j) {
          const char ch = text[tstart[c] + j];
          sextets += (ch != '\n' && ch != '\r' && ch != ' ' && ch != '=');
        }
        const U64 whole = std::min<U64>(sextets / 4 * 3, chunk[c].size() / 3 * 3);
        CHECK(ph.BytesIn(c) >= whole && ph.BytesIn(c) <= chunk[c].size());
      }
    }
  }
  for (U32 c = 0; c < kSlots; ++c) CHECK(finished[c]);
  // the arena: the chunks where they belong, every guard byte as it was
  {
    std::vector<U8> expect(alen, 0xEE);
    for (U32 c = 0; c < kSlots; ++c) std::copy(chunk[c].begin(), chunk[c].end(), expect.begin() + ostart[c]);
    CHECK(arena == expect);
  }

  // Reset drops pending text; a wrong hash string and a text that decodes to more than the chunk
  {
    std::vector<U8> verdicts;
    std::vector<U32> sizes;
    PieceHasher::V_TextPiece one(1);
    one[0].m_slot = 1;
    one[0].m_text_offset = tstart[1];
    one[0].m_text_len = 10;  // two groups and two sextets pending
    one[0].m_out_offset = ostart[1];
    one[0].m_chunk_size = 56;
    CHECK(ph.UpdateText(text.data(), text.size(), one, arena.data(), arena.size(), {std::string()}, verdicts, &sizes) ==
          Error::NO_ERROR_LBF);
    CHECK(ph.BytesIn(1) == 6);
    ph.Reset(1);
    CHECK(ph.BytesIn(1) == 0);
    one[0].m_text_len = tlen[1];
    one[0].m_last = true;
    CHECK(ph.UpdateText(text.data(), text.size(), one, arena.data(), arena.size(), {want[1]}, verdicts, &sizes) ==
          Error::NO_ERROR_LBF);
    CHECK(verdicts.size() == 1 && verdicts[0] == 1 && sizes[0] == 56);  // the pending sextets were dropped
    CHECK(ph.UpdateText(text.data(), text.size(), one, arena.data(), arena.size(), {want[0]}, verdicts, &sizes) ==
          Error::NO_ERROR_LBF);
    CHECK(verdicts[0] == 0 && sizes[0] == 56);
    one[0].m_chunk_size = 50;  // the text decodes to 56
    CHECK(ph.UpdateText(text.data(), text.size(), one, arena.data(), arena.size(), {want[1]}, verdicts, nullptr) ==
          Error::NO_ERROR_LBF);
    CHECK(verdicts[0] == 0);
    one[0].m_last = false;
    CHECK(ph.UpdateText(text.data(), text.size(), one, arena.data(), arena.size(), {want[1]}, verdicts, &sizes) ==
          Error::NO_ERROR_LBF);
    CHECK(ph.BytesIn(1) == 56);  // the true count, past the chunk's size
    ph.Reset(1);
    CHECK(ph.BytesIn(kSlots) == 0);
    std::vector<U8> expect(alen, 0xEE);
    for (U32 c = 0; c < kSlots; ++c) std::copy(chunk[c].begin(), chunk[c].end(), expect.begin() + ostart[c]);
    CHECK(arena == expect);  // a slot of 50 bytes got bytes 0..49 again, nothing past them
  }
  // refused: two pieces of one slot, no such slot, text outside, a slot outside the arena, no hash string
  {
    std::vector<U8> verdicts;
    const V_String none(2);
    PieceHasher::V_TextPiece two(2);
    two[0].m_slot = two[1].m_slot = 2;
    CHECK(ph.UpdateText(text.data(), text.size(), two, arena.data(), arena.size(), none, verdicts, nullptr) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_slot = kSlots;
    CHECK(ph.UpdateText(text.data(), text.size(), two, arena.data(), arena.size(), none, verdicts, nullptr) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_slot = 1;
    two[1].m_text_offset = text.size();
    two[1].m_text_len = 1;
    CHECK(ph.UpdateText(text.data(), text.size(), two, arena.data(), arena.size(), none, verdicts, nullptr) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_text_offset = 0;
    two[1].m_out_offset = arena.size();
    two[1].m_chunk_size = 1;
    CHECK(ph.UpdateText(text.data(), text.size(), two, arena.data(), arena.size(), none, verdicts, nullptr) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_out_offset = 0;
    two[1].m_last = true;
    CHECK(ph.UpdateText(text.data(), text.size(), two, arena.data(), arena.size(), none, verdicts, nullptr) ==
          Error::UNKNOWN_ERROR_LBF);
    CHECK(ph.BytesIn(1) == 0 && ph.BytesIn(2) == 0);
  }

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("piece_text_tests OK\n");
  return 0;
}
