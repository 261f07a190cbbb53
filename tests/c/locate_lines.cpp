// locate_lines.cpp -- PeerWire::LocateSendChunk and PeerWire::EncodeSendChunk
// behind a record protocol, so that tests/test_wire_frames_cpu.py can hold
// tests/wire_frame_model.py (the CPU model of lbf_wire_send_chunks_launch)
// against the C++ itself.
//
//   locate_lines locate < records     one frame per record
//   locate_lines encode < records     name, decimal index and data as three records per frame
//
// A record is a 32-bit little-endian length and that many bytes.
//   locate: "0", or "1 <index> <b64 offset> <b64 length> <hex of o_filename, - if empty>".
//   encode: the hex of EncodeSendChunk's frame.
#include <stdint.h>
#include <stdlib.h>

#include <iostream>
#include <string>

#include "libBitFlood/PeerWire.H"

using namespace libBitFlood;

static bool record(std::string& out) {
  unsigned char n[4];
  if (!std::cin.read(reinterpret_cast<char*>(n), 4)) return false;
  const uint32_t len = n[0] | n[1] << 8 | n[2] << 16 | (uint32_t)n[3] << 24;
  out.resize(len);
  return len == 0 || (bool)std::cin.read(&out[0], len);
}

static std::string hex(const std::string& s) {
  static const char* d = "0123456789abcdef";
  std::string o;
  for (unsigned char c : s) {
    o.push_back(d[c >> 4]);
    o.push_back(d[c & 15]);
  }
  return o.empty() ? "-" : o;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  std::string frame, name, index, data;
  if (mode == "locate") {
    while (record(frame)) {
      std::string file;
      U32 idx = 0;
      size_t off = 0, len = 0;
      // an exact copy: a read past the frame is a read past the allocation
      char* exact = (char*)malloc(frame.size() ? frame.size() : 1);
      frame.copy(exact, frame.size());
      if (PeerWire::LocateSendChunk(exact, frame.size(), file, idx, off, len))
        std::cout << "1 " << idx << ' ' << off << ' ' << len << ' ' << hex(file) << '\n';
      else
        std::cout << "0\n";
      free(exact);
    }
    return 0;
  }
  if (mode == "encode") {
    while (record(name) && record(index) && record(data))
      std::cout << hex(PeerWire::EncodeSendChunk(name, (U32)strtoul(index.c_str(), nullptr, 10),
                                                 reinterpret_cast<const U8*>(data.data()), (U32)data.size()))
                << '\n';
    return 0;
  }
  std::cerr << "usage: locate_lines locate|encode < records\n";
  return 2;
}
