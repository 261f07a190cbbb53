// PieceHasher.cpp -- libBitFlood::PieceHasher: per-slot resumable SHA-1 states
// fed through lbf_sha1_update_batch, one GPU call per Update().
#include "libBitFlood/PieceHasher.H"

#include "lbf_hash.h"
#include "libBitFlood/Encoder.H"

namespace libBitFlood {

PieceHasher::PieceHasher(U32 i_slots, lbf_ctx* i_ctx)
    : m_ctx(i_ctx), m_slots(i_slots), m_states(new lbf_sha1_state[i_slots ? i_slots : 1]) {
  lbf_sha1_state_init(m_states.get(), m_slots);
}

PieceHasher::~PieceHasher() {}

std::shared_ptr<lbf_ctx> PieceHasher::Ctx() const {
  if (m_ctx) return std::shared_ptr<lbf_ctx>(m_ctx, [](lbf_ctx*) {});  // the caller owns it
  return Encoder::SharedContext();
}

Error::ErrorCode PieceHasher::Update(const U8* i_arena, U64 i_arena_len, const V_Piece& i_pieces,
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
  if (lbf_sha1_update_batch(held.get(), m_states.get(), m_slots, slot.data(), i_arena ? i_arena : &kEmpty,
                            i_arena ? i_arena_len : 0, offs.data(), sizes.data(), last.data(), n, digests.data(),
                            nullptr, nullptr) != LBF_OK)
    return Error::UNKNOWN_ERROR_LBF;
  for (U64 k = 0; k < n; ++k) {
    if (!last[k]) continue;
    char s[28];
    lbf_b64_27(&digests[20 * k], s);
    o_hashes[k].assign(s, 27);
  }
  return Error::NO_ERROR_LBF;
}

U64 PieceHasher::BytesIn(U32 i_slot) const { return i_slot < m_slots ? m_states[i_slot].total : 0; }

void PieceHasher::Reset(U32 i_slot) {
  if (i_slot < m_slots) lbf_sha1_state_init(&m_states[i_slot], 1);
}

}  // namespace libBitFlood
