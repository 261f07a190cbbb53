// PieceHasher.cpp -- libBitFlood::PieceHasher: per-slot resumable SHA-1 states
// fed through lbf_sha1_update_batch, one GPU call per Update(), and per-slot
// base64 decoder states beside them fed through lbf_b64_update_batch, one GPU
// call per UpdateText(), and per-slot base64 encoder states fed through
// lbf_b64_encode_update_batch, one GPU call per UpdateEncode().  UpdateSeq() and
// UpdateTextSeq() are Update() and UpdateText() through lbf_sha1_update_seq_batch
// and lbf_b64_update_seq_batch: several pieces per slot, in the caller's order.
#include "libBitFlood/PieceHasher.H"

#include "lbf_hash.h"
#include "libBitFlood/Encoder.H"

namespace libBitFlood {

PieceHasher::PieceHasher(U32 i_slots, lbf_ctx* i_ctx)
    : m_ctx(i_ctx),
      m_slots(i_slots),
      m_states(new lbf_sha1_state[i_slots ? i_slots : 1]),
      m_text_states(new lbf_b64_state[i_slots ? i_slots : 1]),
      m_enc_states(new lbf_b64_enc_state[i_slots ? i_slots : 1]) {
  lbf_sha1_state_init(m_states.get(), m_slots);
  lbf_b64_state_init(m_text_states.get(), m_slots);
  lbf_b64_enc_state_init(m_enc_states.get(), m_slots, LBF_B64_LAYOUT_XMLRPC);
}

PieceHasher::~PieceHasher() {}

std::shared_ptr<lbf_ctx> PieceHasher::Ctx() const {
  if (m_ctx) return std::shared_ptr<lbf_ctx>(m_ctx, [](lbf_ctx*) {});  // the caller owns it
  return Encoder::SharedContext();
}

Error::ErrorCode PieceHasher::Update(const U8* i_arena, U64 i_arena_len, const V_Piece& i_pieces,
                                     V_String& o_hashes) {
  return UpdateBy(false, i_arena, i_arena_len, i_pieces, o_hashes);
}

Error::ErrorCode PieceHasher::UpdateSeq(const U8* i_arena, U64 i_arena_len, const V_Piece& i_pieces,
                                        V_String& o_hashes) {
  return UpdateBy(true, i_arena, i_arena_len, i_pieces, o_hashes);
}

Error::ErrorCode PieceHasher::UpdateBy(bool i_seq, const U8* i_arena, U64 i_arena_len, const V_Piece& i_pieces,
                                       V_String& o_hashes) {
  const U64 n = i_pieces.size();
  o_hashes.assign(n, std::string());
  if (n == 0) return Error::NO_ERROR_LBF;
  const std::shared_ptr<lbf_ctx> held = Ctx();  // alive for the whole call
  if (!held) return Error::UNKNOWN_ERROR_LBF;
  V_U32 slot(n), sizes(n);
  V_U64 offs(n);
  V_U8 last(n), digests(20 * n);
  for (U64 k = 0; k < n; ++k) {
    slot[k] = i_pieces[k].m_slot;
    offs[k] = i_pieces[k].m_offset;
    sizes[k] = i_pieces[k].m_size;
    last[k] = i_pieces[k].m_last ? 1 : 0;
  }
  static const U8 kEmpty = 0;  // an empty arena still gets a real address
  const auto call = i_seq ? lbf_sha1_update_seq_batch : lbf_sha1_update_batch;
  if (call(held.get(), m_states.get(), m_slots, slot.data(), i_arena ? i_arena : &kEmpty, i_arena ? i_arena_len : 0,
           offs.data(), sizes.data(), last.data(), n, digests.data(), nullptr, nullptr) != LBF_OK)
    return Error::UNKNOWN_ERROR_LBF;
  for (U64 k = 0; k < n; ++k) {
    if (!last[k]) continue;
    char s[28];
    lbf_b64_27(&digests[20 * k], s);
    o_hashes[k].assign(s, 27);
  }
  return Error::NO_ERROR_LBF;
}

Error::ErrorCode PieceHasher::UpdateText(const char* i_text, U64 i_text_len, const V_TextPiece& i_pieces,
                                         U8* io_arena, U64 i_arena_len, const V_String& i_expected_hashes,
                                         std::vector<U8>& o_verdicts, std::vector<U32>* o_sizes) {
  return UpdateTextBy(false, i_text, i_text_len, i_pieces, io_arena, i_arena_len, i_expected_hashes, o_verdicts,
                      o_sizes);
}

Error::ErrorCode PieceHasher::UpdateTextSeq(const char* i_text, U64 i_text_len, const V_TextPiece& i_pieces,
                                            U8* io_arena, U64 i_arena_len, const V_String& i_expected_hashes,
                                            std::vector<U8>& o_verdicts, std::vector<U32>* o_sizes) {
  return UpdateTextBy(true, i_text, i_text_len, i_pieces, io_arena, i_arena_len, i_expected_hashes, o_verdicts,
                      o_sizes);
}

Error::ErrorCode PieceHasher::UpdateTextBy(bool i_seq, const char* i_text, U64 i_text_len,
                                           const V_TextPiece& i_pieces, U8* io_arena, U64 i_arena_len,
                                           const V_String& i_expected_hashes, std::vector<U8>& o_verdicts,
                                           std::vector<U32>* o_sizes) {
  const U64 n = i_pieces.size();
  o_verdicts.assign(n, 0);
  if (o_sizes) o_sizes->assign(n, 0);
  if (n == 0) return Error::NO_ERROR_LBF;
  if (i_expected_hashes.size() != n) return Error::UNKNOWN_ERROR_LBF;
  const std::shared_ptr<lbf_ctx> held = Ctx();  // alive for the whole call
  if (!held) return Error::UNKNOWN_ERROR_LBF;
  V_U32 slot(n), lens(n), caps(n), sizes(n, 0);
  V_U64 toffs(n), ooffs(n);
  V_U8 last(n), expected(20 * n, 0);
  for (U64 k = 0; k < n; ++k) {
    const TextPiece& p = i_pieces[k];
    slot[k] = p.m_slot;
    toffs[k] = p.m_text_offset;
    lens[k] = p.m_text_len;
    ooffs[k] = p.m_out_offset;
    caps[k] = p.m_chunk_size;
    last[k] = p.m_last ? 1 : 0;
    // a string that is no hash string can match nothing: the call fails before any GPU work
    if (p.m_last && lbf_b64_27_decode(i_expected_hashes[k].data(), i_expected_hashes[k].size(), &expected[20 * k]) !=
                        LBF_OK)
      return Error::UNKNOWN_ERROR_LBF;
  }
  static const char kNoText = 0;  // empty text still gets a real address
  const auto call = i_seq ? lbf_b64_update_seq_batch : lbf_b64_update_batch;
  if (call(held.get(), m_text_states.get(), m_states.get(), m_slots, slot.data(), i_text ? i_text : &kNoText,
           i_text ? i_text_len : 0, toffs.data(), lens.data(), last.data(), n, caps.data(), expected.data(), io_arena,
           io_arena ? i_arena_len : 0, ooffs.data(), sizes.data(), o_verdicts.data()) != LBF_OK)
    return Error::UNKNOWN_ERROR_LBF;
  for (U64 k = 0; k < n; ++k)
    if (!last[k]) o_verdicts[k] = 0;
  if (o_sizes) *o_sizes = sizes;
  return Error::NO_ERROR_LBF;
}

Error::ErrorCode PieceHasher::UpdateEncode(const U8* i_arena, U64 i_arena_len, const V_EncodePiece& i_pieces,
                                           char* io_text, U64 i_text_len, const V_String& i_expected_hashes,
                                           std::vector<U8>& o_verdicts, V_NewText& o_new) {
  const U64 n = i_pieces.size();
  o_verdicts.assign(n, 0);
  o_new.assign(n, NewText());
  if (n == 0) return Error::NO_ERROR_LBF;
  if (i_expected_hashes.size() != n) return Error::UNKNOWN_ERROR_LBF;
  const std::shared_ptr<lbf_ctx> held = Ctx();  // alive for the whole call
  if (!held) return Error::UNKNOWN_ERROR_LBF;
  V_U32 slot(n), sizes(n), caps(n), lens(n, 0);
  V_U64 offs(n), toffs(n), noffs(n, 0);
  V_U8 last(n), expected(20 * n, 0);
  for (U64 k = 0; k < n; ++k) {
    const EncodePiece& p = i_pieces[k];
    slot[k] = p.m_slot;
    offs[k] = p.m_offset;
    sizes[k] = p.m_size;
    last[k] = p.m_last ? 1 : 0;
    toffs[k] = p.m_text_offset;
    caps[k] = p.m_text_cap;
    if (p.m_layout != LAYOUT_XMLRPC && p.m_layout != LAYOUT_FLAT) return Error::UNKNOWN_ERROR_LBF;
    // a string that is no hash string can match nothing: the call fails before any GPU work
    if (p.m_last && lbf_b64_27_decode(i_expected_hashes[k].data(), i_expected_hashes[k].size(), &expected[20 * k]) !=
                        LBF_OK)
      return Error::UNKNOWN_ERROR_LBF;
  }
  // the layout is fixed at a slot's first piece of a chunk; put back if the call is refused
  std::vector<U8> before(n, 0);
  for (U64 k = 0; k < n; ++k) {
    const U32 s = slot[k];
    if (s >= m_slots) continue;  // refused below
    before[k] = m_enc_states[s].layout;
    if (m_enc_states[s].taken == 0 && m_states[s].total == 0) m_enc_states[s].layout = (U8)i_pieces[k].m_layout;
  }
  static const U8 kEmpty = 0;  // an empty arena still gets a real address
  if (lbf_b64_encode_update_batch(held.get(), m_enc_states.get(), m_states.get(), m_slots, slot.data(),
                                  i_arena ? i_arena : &kEmpty, i_arena ? i_arena_len : 0, offs.data(), sizes.data(),
                                  last.data(), n, expected.data(), o_verdicts.data(), io_text, io_text ? i_text_len : 0,
                                  toffs.data(), caps.data(), noffs.data(), lens.data(), nullptr) != LBF_OK) {
    for (U64 k = n; k-- > 0;)
      if (slot[k] < m_slots) m_enc_states[slot[k]].layout = before[k];
    return Error::UNKNOWN_ERROR_LBF;
  }
  for (U64 k = 0; k < n; ++k) {
    if (!last[k]) o_verdicts[k] = 0;
    o_new[k].m_offset = noffs[k];
    o_new[k].m_len = lens[k];
  }
  return Error::NO_ERROR_LBF;
}

U64 PieceHasher::BytesIn(U32 i_slot) const {
  if (i_slot >= m_slots) return 0;
  // a slot fed text counts what the text decoded to, the bytes past the chunk's size included
  return m_states[i_slot].total > m_text_states[i_slot].decoded ? m_states[i_slot].total
                                                                : m_text_states[i_slot].decoded;
}

void PieceHasher::Reset(U32 i_slot) {
  if (i_slot >= m_slots) return;
  lbf_sha1_state_init(&m_states[i_slot], 1);
  lbf_b64_state_init(&m_text_states[i_slot], 1);
  lbf_b64_enc_state_init(&m_enc_states[i_slot], 1, LBF_B64_LAYOUT_XMLRPC);
}

}  // namespace libBitFlood
