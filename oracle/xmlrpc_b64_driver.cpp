// xmlrpc_b64_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs xmlrpc++ 0.7's own
// base64 codec (its header is found through -I, see the Makefile's `ref`
// target; nothing of it is kept here) so that its outputs can be recorded as
// a fixture (tests/golden/make_xmlrpc_b64_fixture.py).
//
//   xmlrpc_b64_driver get|put < lines
//
// Each input line is one hex-encoded byte string ("-" for the empty one).
//   get: the line is a text; it is decoded as XmlRpcValue::binaryFromXml does
//        (XmlRpcValue.cpp:429-432: a back inserter into a vector, iostatus 0)
//        and the answer is "hex-of-output iostatus consumed", consumed = how
//        far the returned iterator went.
//   put: the line is a chunk; the answer is the hex of the encoder's output,
//        called as XmlRpcValue::binaryToXml does (XmlRpcValue.cpp:442-446).
#include <ios>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "base64.h"

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

template <class C>
static std::string hex(const C& bytes) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (auto b : bytes) {
    s.push_back(d[((unsigned char)b) >> 4]);
    s.push_back(d[((unsigned char)b) & 15]);
  }
  return s.empty() ? "-" : s;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode != "get" && mode != "put") {
    std::cerr << "usage: xmlrpc_b64_driver get|put < hex lines\n";
    return 2;
  }
  std::string line, in;
  while (std::getline(std::cin, line)) {
    if (!unhex(line, in)) {
      std::cerr << "bad hex line\n";
      return 2;
    }
    int iostatus = 0;
    if (mode == "get") {
      std::vector<char> bin;
      base64<char> decoder;
      std::back_insert_iterator<std::vector<char> > ins = std::back_inserter(bin);
      std::string::iterator end = decoder.get(in.begin(), in.end(), ins, iostatus);
      std::cout << hex(bin) << ' ' << iostatus << ' ' << (end - in.begin()) << '\n';
    } else {
      std::vector<char> text;
      base64<char> encoder;
      std::back_insert_iterator<std::vector<char> > ins = std::back_inserter(text);
      encoder.put(in.begin(), in.end(), ins, iostatus, base64<>::crlf());
      std::cout << hex(text) << '\n';
    }
  }
  return 0;
}
