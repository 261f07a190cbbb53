// placement.cpp -- environment numbers, the caller's current device, and NUMA
// placement of a worker's staging memory and host threads.
//
// NUMA placement: each worker's pinned staging is
// allocated on its GPU's NUMA node and its host threads (the worker thread of
// a multi-worker job and the staging-copy threads) run on that node's CPUs, so
// the host memcpy/pread writes local DRAM and the DMA engine reads it without
// crossing the socket link.  The node comes from the GPU's PCI bus id
// (/sys/bus/pci/devices/<id>/numa_node); LBF_NUMA=0 turns placement off.  Raw
// syscalls: no libnuma dependency.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <cctype>
#include <cstdio>
#include <cstdlib>

#include "lbf_host.hpp"

namespace lbf {

uint64_t env_u64(const char* name, uint64_t dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  return strtoull(v, nullptr, 10);
}

long env_long(const char* name, long dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  return strtol(v, nullptr, 10);
}

KeepCurrentDevice::KeepCurrentDevice() {
  if (hipGetDevice(&saved) != hipSuccess) saved = -1;
}
KeepCurrentDevice::~KeepCurrentDevice() {
  if (saved >= 0) (void)hipSetDevice(saved);
}

namespace {

constexpr int kMpolDefault = 0, kMpolPreferred = 1;
constexpr unsigned long kMpolFNode = 1, kMpolFAddr = 2;

std::string read_line(const std::string& path) {
  FILE* f = fopen(path.c_str(), "r");
  if (!f) return "";
  char buf[4096];
  std::string out;
  if (fgets(buf, sizeof(buf), f)) out = buf;
  fclose(f);
  while (!out.empty() && (out.back() == '\n' || out.back() == ' ')) out.pop_back();
  return out;
}

std::vector<int> parse_cpulist(const std::string& s) {  // "0-63,128-191"
  std::vector<int> out;
  size_t p = 0;
  while (p < s.size()) {
    char* end = nullptr;
    const long a = strtol(s.c_str() + p, &end, 10);
    if (end == s.c_str() + p) break;
    long b = a;
    p = (size_t)(end - s.c_str());
    if (p < s.size() && s[p] == '-') {
      b = strtol(s.c_str() + p + 1, &end, 10);
      p = (size_t)(end - s.c_str());
    }
    for (long c = a; c <= b && c < CPU_SETSIZE; ++c) out.push_back((int)c);
    if (p < s.size() && s[p] == ',') ++p;
    else break;
  }
  return out;
}

}  // namespace

bool numa_enabled() {
  static const bool on = env_long("LBF_NUMA", 1) != 0;
  return on;
}

int device_numa_node(int device) {
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) return -1;
  std::string id(bus);
  for (char& c : id) c = (char)tolower((unsigned char)c);
  const std::string v = read_line("/sys/bus/pci/devices/" + id + "/numa_node");
  return v.empty() ? -1 : atoi(v.c_str());
}

std::vector<int> node_cpus_allowed(int node) {
  if (node < 0) return {};
  const std::vector<int> cpus = parse_cpulist(read_line("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist"));
  cpu_set_t allowed;
  CPU_ZERO(&allowed);
  if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return {};
  std::vector<int> out;
  for (int c : cpus)
    if (CPU_ISSET(c, &allowed)) out.push_back(c);
  return out;
}

void bind_thread(const std::vector<int>& cpus) {
  if (cpus.empty()) return;
  cpu_set_t set;
  CPU_ZERO(&set);
  for (int c : cpus) CPU_SET(c, &set);
  (void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);  // advisory: a refusal only costs locality
}

PreferNode::PreferNode(int node) {
  old_mode = kMpolDefault;
  if (node < 0 || node >= (int)kMaxNodes) return;
  if (syscall(SYS_get_mempolicy, &old_mode, old_mask, kMaxNodes, nullptr, 0ul) != 0) return;
  unsigned long mask[kMaxNodes / 64] = {};
  mask[node / 64] = 1ul << (node % 64);
  active = syscall(SYS_set_mempolicy, kMpolPreferred, mask, kMaxNodes) == 0;
}

PreferNode::~PreferNode() {
  if (!active) return;
  if (old_mode == kMpolDefault) (void)syscall(SYS_set_mempolicy, kMpolDefault, nullptr, 0ul);
  else (void)syscall(SYS_set_mempolicy, old_mode, old_mask, kMaxNodes);
}

int page_node(const void* p) {
  if (!p) return -1;
  int node = -1;
  if (syscall(SYS_get_mempolicy, &node, nullptr, 0ul, const_cast<void*>(p), kMpolFNode | kMpolFAddr) != 0) return -1;
  return node;
}

}  // namespace lbf
