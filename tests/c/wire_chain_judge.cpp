// wire_chain_judge.cpp -- lbf_wire_frames_launch and lbf_wire_send_chunks_launch
// judged by the C++ they restate (tests/test_gpu_wire_frames.py builds and
// runs it).  The stream is made of PeerWire::EncodeSendChunk /
// FrameSendChunkText / EncodeMethod frames and an unfinished one, the flood
// table comes from Flood::WireTable; every lbf_wire_frame is compared with
// PeerWire::LocateSendChunk on that frame, the binding with a lookup in the
// flood file, and the dense tables with the bound frames in order.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "lbf_hash.h"
#include "libBitFlood/Flood.H"
#include "libBitFlood/PeerWire.H"

using namespace libBitFlood;

#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      return 1;                                                  \
    }                                                            \
  } while (0)
#define OK(call)                                                                   \
  do {                                                                             \
    if ((call) != LBF_OK) {                                                        \
      printf("FAILED %s:%d: %s: %s\n", __FILE__, __LINE__, #call, lbf_last_error()); \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

template <class T>
struct Dev {
  T* p = nullptr;
  size_t n;
  explicit Dev(size_t count, int fill = 0xEE) : n(count) {
    std::vector<uint8_t> h(bytes(), (uint8_t)fill);
    if (lbf_dev_malloc((void**)&p, bytes()) != LBF_OK || lbf_memcpy_h2d(p, h.data(), bytes()) != LBF_OK) p = nullptr;
  }
  ~Dev() { lbf_dev_free(p); }
  size_t bytes() const { return (n ? n : 1) * sizeof(T); }
  int put(const void* src, size_t count) { return lbf_memcpy_h2d(p, src, count * sizeof(T)); }
  std::vector<T> get() const {
    std::vector<T> h(n ? n : 1);
    lbf_memcpy_d2h(h.data(), p, bytes());
    h.resize(n);
    return h;
  }
};

int main() {
  // the flood: two files, the second name needs escaping
  FloodFileSPtr ff(new FloodFile);
  const char* names[2] = {"dir/one.bin", "two <&> \"'.bin"};
  const U32 counts[2] = {3, 2};
  for (int f = 0; f < 2; ++f) {
    FloodFile::FileSPtr file(new FloodFile::File);
    file->m_name = names[f];
    for (U32 k = 0; k < counts[f]; ++k) {
      FloodFile::Chunk c;
      U8 digest[20];
      for (int b = 0; b < 20; ++b) digest[b] = (U8)(17 * f + 5 * k + b);
      char text[28];
      lbf_b64_27(digest, text);
      c.m_hash.assign(text, 27);
      c.m_index = k;
      c.m_size = 40 + k;
      file->m_chunks.push_back(c);
    }
    ff->m_files[file->m_name] = file;
  }
  Flood flood;
  flood.m_floodfile = ff;
  Flood::WireFloodTable t;
  CHECK(flood.WireTable(t) == Error::NO_ERROR_LBF);
  CHECK(t.m_first.size() == 3 && t.m_sizes.size() == 5);

  // the stream
  std::vector<U8> data(100);
  for (size_t i = 0; i < data.size(); ++i) data[i] = (U8)(i * 7 + 1);
  std::string stream;
  using PeerWire::Value;
  stream += PeerWire::EncodeMethod(PeerWire::kNotifyHaveChunk, {Value::Str(names[0]), Value::Int(1)});
  stream += PeerWire::EncodeSendChunk(names[0], 0, data.data(), 40);
  stream += PeerWire::EncodeSendChunk(names[1], 1, data.data(), 41);
  stream += PeerWire::FrameSendChunkText(names[0], 2, "QUJDRA==", 8);  // a flat peer's text
  stream += PeerWire::EncodeSendChunk(names[0], 3, data.data(), 43);   // past the file's chunks
  stream += PeerWire::EncodeSendChunk("three.bin", 0, data.data(), 5);  // not in the flood
  stream += "\n";
  stream += PeerWire::EncodeMethod(PeerWire::kRequestChunk, {PeerWire::Value::Str(names[1]), PeerWire::Value::Int(0)});
  stream += PeerWire::EncodeSendChunk(names[1], 0, data.data(), 0);
  stream += PeerWire::EncodeSendChunk(names[0], 0, data.data(), 40);   // the same chunk again
  const size_t whole = stream.size();
  stream += PeerWire::EncodeSendChunk(names[0], 1, data.data(), 41).substr(0, 150);  // unfinished

  const uint32_t max_frames = 32, max_chunks = 8;
  const size_t lead = 16 + 11;  // the stream at phase 11
  Dev<char> d_buf(lead + stream.size() + 1, '\n');
  CHECK(d_buf.p && lbf_memcpy_h2d(d_buf.p + lead, stream.data(), stream.size()) == LBF_OK);
  const char* d_stream = d_buf.p + lead;
  Dev<uint64_t> d_off(max_frames), d_tail(1), d_toff(max_chunks);
  Dev<uint32_t> d_len(max_frames), d_n(1), d_noff(t.m_nameoffsets.size()), d_first(t.m_first.size()),
      d_sizes(t.m_sizes.size()), d_tlen(max_chunks), d_esz(max_chunks), d_cof(max_chunks), d_fof(max_chunks), d_nloc(1);
  Dev<char> d_names(t.m_names.size());
  Dev<uint8_t> d_exp(t.m_expected.size()), d_dexp(20 * max_chunks);
  Dev<lbf_wire_frame> d_frames(max_frames);
  Dev<uint8_t> d_w1(lbf_wire_frames_launch_work(stream.size())), d_w2(lbf_wire_send_chunks_launch_work(max_frames));
  OK(d_names.put(t.m_names.data(), t.m_names.size()));
  OK(d_noff.put(t.m_nameoffsets.data(), t.m_nameoffsets.size()));
  OK(d_first.put(t.m_first.data(), t.m_first.size()));
  OK(d_sizes.put(t.m_sizes.data(), t.m_sizes.size()));
  OK(d_exp.put(t.m_expected.data(), t.m_expected.size()));

  void* st = nullptr;
  OK(lbf_stream_create(&st));
  OK(lbf_wire_frames_launch(d_stream, stream.size(), d_off.p, d_len.p, max_frames, d_n.p, d_tail.p, d_w1.p, st));
  OK(lbf_wire_send_chunks_launch(d_stream, stream.size(), d_off.p, d_len.p, max_frames, d_n.p, d_names.p, d_noff.p,
                                 d_first.p, 2, d_sizes.p, d_exp.p, (uint32_t)t.m_sizes.size(), d_frames.p, d_toff.p,
                                 d_tlen.p, d_esz.p, d_dexp.p, d_cof.p, d_fof.p, max_chunks, d_nloc.p, d_w2.p, st));
  OK(lbf_stream_synchronize(st));
  OK(lbf_stream_destroy(st));

  // the split against memchr
  const std::vector<uint64_t> off = d_off.get(), toff = d_toff.get();
  const std::vector<uint32_t> len = d_len.get(), tlen = d_tlen.get(), esz = d_esz.get(), cof = d_cof.get(),
                              fof = d_fof.get();
  const std::vector<uint8_t> dexp = d_dexp.get();
  const std::vector<lbf_wire_frame> frames = d_frames.get();
  uint32_t found = 0;
  size_t start = 0;
  while (const void* nl = memchr(stream.data() + start, '\n', stream.size() - start)) {
    const size_t p = (size_t)((const char*)nl - stream.data());
    CHECK(found < max_frames && off[found] == start && len[found] == p - start);
    start = p + 1;
    ++found;
  }
  CHECK(found == 10 && d_n.get()[0] == found && d_tail.get()[0] == start && start == whole);

  // every frame against LocateSendChunk, the binding against the flood file
  uint32_t located = 0;
  for (uint32_t i = 0; i < found; ++i) {
    const lbf_wire_frame& fr = frames[i];
    std::string name;
    U32 index = 0;
    size_t b64_off = 0, b64_len = 0;
    if (!PeerWire::LocateSendChunk(stream.data() + off[i], len[i], name, index, b64_off, b64_len)) {
      CHECK(fr.kind == LBF_FRAME_OTHER && fr.text_offset == 0 && fr.name_offset == 0 && fr.text_len == 0 &&
            fr.name_len == 0 && fr.index == 0);
      continue;
    }
    CHECK(fr.text_offset == off[i] + b64_off && fr.text_len == b64_len && fr.index == index);
    CHECK(fr.name_offset + fr.name_len <= stream.size());
    CHECK(PeerWire::XmlDecode(stream.substr(fr.name_offset, fr.name_len)) == name);
    uint32_t first = 0, chunk = UINT32_MAX;
    for (const auto& kv : ff->m_files) {
      if (kv.first == name && index < kv.second->m_chunks.size()) chunk = first + index;
      first += (uint32_t)kv.second->m_chunks.size();
    }
    CHECK(fr.kind == (chunk == UINT32_MAX ? LBF_FRAME_SEND_CHUNK_UNBOUND : LBF_FRAME_SEND_CHUNK));
    if (chunk == UINT32_MAX) continue;
    CHECK(located < max_chunks);
    CHECK(toff[located] == fr.text_offset && tlen[located] == fr.text_len && esz[located] == t.m_sizes[chunk] &&
          cof[located] == chunk && fof[located] == i);
    CHECK(memcmp(&dexp[20 * located], &t.m_expected[20 * chunk], 20) == 0);
    ++located;
  }
  CHECK(located == 5 && d_nloc.get()[0] == located);
  for (uint32_t j = located; j < max_chunks; ++j) {
    CHECK(toff[j] == 0 && tlen[j] == 0 && esz[j] == 0 && cof[j] == UINT32_MAX && fof[j] == UINT32_MAX);
    for (int b = 0; b < 20; ++b) CHECK(dexp[20 * j + b] == 0);
  }
  for (uint32_t i = found; i < max_frames; ++i) CHECK(frames[i].kind == 0xEEEEEEEEu && off[i] == 0xEEEEEEEEEEEEEEEEull);
  printf("wire_chain_judge: OK (%u frames, %u bound)\n", found, located);
  return 0;
}
