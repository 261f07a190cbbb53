// b64get_lines.cpp -- PeerWire::Base64Get / Base64Put over the line protocol
// of oracle/xmlrpc_b64_driver.cpp, so that tests/test_wire_layouts.py can hold
// the host's restatement of xmlrpc++'s codec against outputs recorded from the
// codec itself (tests/golden/xmlrpc07_base64_get.json).
//
//   b64get_lines get|put < lines
//
// Each input line is one hex-encoded byte string ("-" for the empty one).
//   get: the hex of Base64Get's output (capacity: the text's length, which no
//        decode exceeds).
//   put: the hex of Base64Put's text.
#include <iostream>
#include <string>
#include <vector>

#include "libBitFlood/PeerWire.H"

using namespace libBitFlood;

static bool unhex(const std::string& line, std::string& out) {
  out.clear();
  if (line == "-") return true;
  if (line.size() % 2) return false;
  auto nib = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; };
  for (size_t i = 0; i < line.size(); i += 2) {
    const int h = nib(line[i]), l = nib(line[i + 1]);
    if (h < 0 || l < 0) return false;
    out.push_back((char)(h * 16 + l));
  }
  return true;
}

static std::string hex(const unsigned char* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s.push_back(d[p[i] >> 4]);
    s.push_back(d[p[i] & 15]);
  }
  return s.empty() ? "-" : s;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode != "get" && mode != "put") {
    std::cerr << "usage: b64get_lines get|put < hex lines\n";
    return 2;
  }
  std::string line, in;
  while (std::getline(std::cin, line)) {
    if (!unhex(line, in)) {
      std::cerr << "bad hex line\n";
      return 2;
    }
    const unsigned char* src = reinterpret_cast<const unsigned char*>(in.data());
    if (mode == "get") {
      std::vector<unsigned char> out(in.size() + 1);
      const long n = PeerWire::Base64Get(in.data(), in.size(), out.data(), out.size());
      if (n < 0) {
        std::cerr << "Base64Get: capacity\n";
        return 1;
      }
      std::cout << hex(out.data(), (size_t)n) << '\n';
    } else {
      std::string text;
      PeerWire::Base64Put(in.empty() ? nullptr : src, in.size(), text);
      std::cout << hex(reinterpret_cast<const unsigned char*>(text.data()), text.size()) << '\n';
    }
  }
  return 0;
}
