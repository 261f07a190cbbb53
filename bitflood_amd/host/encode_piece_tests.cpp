// encode_piece_tests.cpp -- libBitFlood::PieceHasher::UpdateEncode on the GPU
// (run by tests/test_gpu_piece_encode.py): three chunks whose hash strings are
// recorded in tests/golden/kat.json ("abc", the 56-byte NIST message, 64 KiB of
// zeros) are read in pieces over two calls and leave as base64 text, one slot in
// xmlrpc++'s lines and two unbroken, checked against strings computed on the
// host (PeerWire::Base64Put); then a Reset in mid-chunk, a wrong hash string, a
// slot too small, and the refusals.
//   lbf_encode_piece_tests
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

// The chunk's text as the frame carries it: xmlrpc++'s lines with the newline
// framed as a space, or the same characters unbroken.
static std::string HostText(const std::vector<U8>& chunk, PieceHasher::Layout layout) {
  std::string lines, out;
  PeerWire::Base64Put(chunk.data(), chunk.size(), lines);
  for (char c : lines) {
    if (c != '\n') out.push_back(c);
    else if (layout == PieceHasher::LAYOUT_XMLRPC) out.push_back(' ');
  }
  return out;
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
  const U32 kSlots = 3, kGuard = 5;
  const PieceHasher::Layout layout[3] = {PieceHasher::LAYOUT_FLAT, PieceHasher::LAYOUT_XMLRPC,
                                         PieceHasher::LAYOUT_FLAT};
  // the chunks follow one another in the arena; the text slots lie with guard bytes around each
  std::vector<U8> arena;
  std::vector<U64> astart(kSlots), tstart(kSlots);
  std::vector<std::string> text_of(kSlots);
  U64 tlen = kGuard;
  for (U32 c = 0; c < kSlots; ++c) {
    astart[c] = arena.size();
    arena.insert(arena.end(), chunk[c].begin(), chunk[c].end());
    text_of[c] = HostText(chunk[c], layout[c]);
    tstart[c] = tlen;
    tlen += text_of[c].size() + kGuard;
  }
  CHECK(text_of[1].size() == 77 && text_of[1][72] == ' ' && text_of[0] == "YWJj");
  std::string text(tlen, '\xEE'), expect(tlen, '\xEE');

  PieceHasher ph(kSlots);
  // two calls: the first pieces split a group (1, 55 and 30,001 bytes), the second ones end the chunks
  const U32 first[3] = {1, 55, 30001};
  for (int call = 0; call < 2; ++call) {
    PieceHasher::V_EncodePiece pieces;
    V_String expected;
    for (U32 k = 0; k < kSlots; ++k) {
      const U32 c = (k + call) % kSlots;  // the order of the slots changes from call to call
      PieceHasher::EncodePiece p;
      p.m_slot = c;
      p.m_offset = astart[c] + (call ? first[c] : 0);
      p.m_size = call ? (U32)chunk[c].size() - first[c] : first[c];
      p.m_last = call == 1;
      p.m_text_offset = tstart[c];
      p.m_text_cap = (U32)text_of[c].size();
      p.m_layout = call ? PieceHasher::LAYOUT_XMLRPC : layout[c];  // counts at the chunk's first piece only
      if (c == 1) p.m_layout = layout[c];
      pieces.push_back(p);
      expected.push_back(p.m_last ? want[c] : std::string());
    }
    std::vector<U8> verdicts;
    PieceHasher::V_NewText fresh;
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), pieces, &text[0], text.size(), expected, verdicts, fresh) ==
          Error::NO_ERROR_LBF);
    CHECK(verdicts.size() == pieces.size() && fresh.size() == pieces.size());
    for (size_t k = 0; k < pieces.size() && k < verdicts.size() && k < fresh.size(); ++k) {
      const U32 c = pieces[k].m_slot;
      const U64 groups = first[c] / 3;  // whole groups of the first piece
      const U64 cut = 4 * groups + (layout[c] == PieceHasher::LAYOUT_XMLRPC ? groups / 18 : 0);
      const U64 from = call ? cut : 0, to = call ? text_of[c].size() : cut;
      CHECK(fresh[k].m_offset == tstart[c] + from && fresh[k].m_len == to - from);
      expect.replace(tstart[c] + from, to - from, text_of[c], from, to - from);
      CHECK(verdicts[k] == (call ? 1 : 0));
      CHECK(ph.BytesIn(c) == (call ? 0 : first[c]));  // a finished chunk: the slot starts its next one
    }
    CHECK(text == expect);  // the characters so far where they belong, every other byte as it was
  }

  // Reset in mid-chunk drops the carried bytes and the layout; then a wrong hash string, and a slot too small
  {
    std::vector<U8> verdicts;
    PieceHasher::V_NewText fresh;
    PieceHasher::V_EncodePiece one(1);
    one[0].m_slot = 1;
    one[0].m_offset = astart[1];
    one[0].m_size = 10;  // three groups and a byte carried
    one[0].m_text_offset = tstart[1];
    one[0].m_text_cap = (U32)text_of[1].size();
    one[0].m_layout = PieceHasher::LAYOUT_FLAT;
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), one, &text[0], text.size(), {std::string()}, verdicts, fresh) ==
          Error::NO_ERROR_LBF);
    CHECK(ph.BytesIn(1) == 10 && fresh[0].m_len == 12);
    ph.Reset(1);
    CHECK(ph.BytesIn(1) == 0);
    one[0].m_size = 56;
    one[0].m_last = true;
    one[0].m_layout = PieceHasher::LAYOUT_XMLRPC;
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), one, &text[0], text.size(), {want[1]}, verdicts, fresh) ==
          Error::NO_ERROR_LBF);
    CHECK(verdicts[0] == 1 && fresh[0].m_offset == tstart[1] && fresh[0].m_len == 77);  // nothing carried over
    CHECK(text == expect);
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), one, &text[0], text.size(), {want[0]}, verdicts, fresh) ==
          Error::NO_ERROR_LBF);
    CHECK(verdicts[0] == 0 && fresh[0].m_len == 77);
    one[0].m_text_cap = 70;  // the text is 77 characters
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), one, &text[0], text.size(), {want[1]}, verdicts, fresh) ==
          Error::NO_ERROR_LBF);
    CHECK(verdicts[0] == 0 && fresh[0].m_len == 70);
    CHECK(text == expect);  // a slot of 70 characters got characters 0..69 again, nothing past them
    CHECK(ph.BytesIn(kSlots) == 0);
  }
  // refused: two pieces of one slot, no such slot, a piece outside the arena, a slot outside the text, no hash string
  {
    std::vector<U8> verdicts;
    PieceHasher::V_NewText fresh;
    const V_String none(2);
    PieceHasher::V_EncodePiece two(2);
    two[0].m_slot = two[1].m_slot = 2;
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), two, &text[0], text.size(), none, verdicts, fresh) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_slot = kSlots;
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), two, &text[0], text.size(), none, verdicts, fresh) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_slot = 1;
    two[1].m_offset = arena.size();
    two[1].m_size = 1;
    two[1].m_layout = PieceHasher::LAYOUT_FLAT;
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), two, &text[0], text.size(), none, verdicts, fresh) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_offset = 0;
    two[1].m_text_offset = text.size();
    two[1].m_text_cap = 1;
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), two, &text[0], text.size(), none, verdicts, fresh) ==
          Error::UNKNOWN_ERROR_LBF);
    two[1].m_text_offset = 0;
    two[1].m_text_cap = 0;
    two[1].m_last = true;
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), two, &text[0], text.size(), none, verdicts, fresh) ==
          Error::UNKNOWN_ERROR_LBF);
    CHECK(ph.BytesIn(1) == 0 && ph.BytesIn(2) == 0);
    CHECK(text == expect);
    // the refused calls left nothing behind: slot 1's next chunk comes out whole
    PieceHasher::V_EncodePiece one(1);
    one[0].m_slot = 1;
    one[0].m_offset = astart[1];
    one[0].m_size = 56;
    one[0].m_last = true;
    one[0].m_text_offset = tstart[1];
    one[0].m_text_cap = 77;
    CHECK(ph.UpdateEncode(arena.data(), arena.size(), one, &text[0], text.size(), {want[1]}, verdicts, fresh) ==
          Error::NO_ERROR_LBF);
    CHECK(verdicts[0] == 1 && fresh[0].m_len == 77 && text == expect);
  }

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("encode_piece_tests OK\n");
  return 0;
}
