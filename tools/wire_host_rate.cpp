// wire_host_rate.cpp -- the host steps lbf_wire_frames_launch and
// lbf_wire_send_chunks_launch replace, timed on one core for
// tools/wire_frames_rate.py: memchr('\n') over a stream read from a file, then
// PeerWire::LocateSendChunk on every frame.
//
//   wire_host_rate <stream file>   prints "<frames> <located> <median microseconds of 5 passes>"
#include <string.h>

#include <algorithm>
#include <chrono>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "libBitFlood/PeerWire.H"

using namespace libBitFlood;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  const std::string s((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::vector<double> us;
  size_t frames = 0, located = 0;
  for (int pass = 0; pass < 5; ++pass) {
    frames = located = 0;
    const auto t0 = std::chrono::steady_clock::now();
    size_t start = 0;
    while (const void* nl = memchr(s.data() + start, '\n', s.size() - start)) {
      const size_t end = (size_t)((const char*)nl - s.data());
      std::string name;
      U32 index;
      size_t off, len;
      located += PeerWire::LocateSendChunk(s.data() + start, end - start, name, index, off, len) ? 1 : 0;
      ++frames;
      start = end + 1;
    }
    us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(us.begin(), us.end());
  std::cout << frames << ' ' << located << ' ' << us[2] << '\n';
  return 0;
}
