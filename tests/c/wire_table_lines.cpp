// wire_table_lines.cpp -- Flood::WireTable over a flood described on stdin, so
// that tests/test_wire_frames_cpu.py can hold it against
// bitflood_amd.wire_flood_table.  No GPU: the flood is never initialised.
//
// Input lines:  "F <hex name, - if empty>"  opens a file,
//               "C <index> <size> <hash string>"  adds a chunk to it, in any order.
// Output: "ok" or "error", then one line each, hex or numbers: names,
// nameoffsets, first, sizes, expected.
#include <iostream>
#include <sstream>
#include <string>

#include "libBitFlood/Flood.H"

using namespace libBitFlood;

static std::string unhex(const std::string& h) {
  std::string o;
  if (h == "-") return o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return o;
}

template <class V>
static void numbers(const V& v) {
  for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? " " : "") << (unsigned long)v[i];
  std::cout << '\n';
}

int main() {
  FloodFileSPtr ff(new FloodFile);
  FloodFile::FileSPtr cur;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "F") {
      std::string name;
      in >> name;
      cur = FloodFile::FileSPtr(new FloodFile::File);
      cur->m_name = unhex(name);
      ff->m_files[cur->m_name] = cur;
    } else if (kind == "C" && cur) {
      FloodFile::Chunk c;
      in >> c.m_index >> c.m_size >> c.m_hash;
      cur->m_chunks.push_back(c);
    }
  }
  Flood flood;
  Flood::WireFloodTable t;
  const bool none = flood.WireTable(t) != Error::NO_ERROR_LBF;  // no flood file yet
  flood.m_floodfile = ff;
  const Error::ErrorCode rc = flood.WireTable(t);
  std::cout << (none && rc == Error::NO_ERROR_LBF ? "ok" : "error") << '\n';
  static const char* d = "0123456789abcdef";
  std::string names;
  for (unsigned char c : t.m_names) {
    names.push_back(d[c >> 4]);
    names.push_back(d[c & 15]);
  }
  std::cout << (names.empty() ? "-" : names) << '\n';
  numbers(t.m_nameoffsets);
  numbers(t.m_first);
  numbers(t.m_sizes);
  numbers(t.m_expected);
  return 0;
}
