// wire_frames.hpp -- the geometry and the work layouts of lbf_wire_frames_launch
// and lbf_wire_send_chunks_launch (wire_frames.hip): a raw receive stream in
// device memory split into frames on '\n', PeerWire::LocateSendChunk run on
// every frame, the located frames bound to the flood's chunks and compacted
// into the dense tables lbf_b64_verify_launch reads.  Not part of the ABI.
// DESIGN.md §4.11.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lbf_hash.h"

namespace lbf {
namespace wiref {

// wire_split_count_kernel / wire_split_scatter_kernel: the lanes of a
// workgroup and the bytes of the stream it takes, 16 a lane, counted from the
// aligned 16-byte block that holds the stream's first byte.
constexpr uint32_t kSplitLanes = 256;
constexpr uint32_t kSplitBlock = 4096;
// wire_locate_kernel: one workgroup per frame; the search primitive takes
// kSearchTrip bytes a trip, 16 a lane, counted from the aligned 16-byte block
// that holds the byte the search starts at.
constexpr uint32_t kLocateLanes = 256;
constexpr uint32_t kSearchTrip = 4096;
// wire_bind_kernel / wire_bind_count_kernel / wire_bind_scatter_kernel: frames (lanes) a workgroup.
constexpr uint32_t kBindBlock = 256;
// wire_scan_kernel: the lanes of its one workgroup, and the counts it takes a trip.
constexpr uint32_t kScanWidth = 1024;
// A longer frame is LBF_FRAME_OTHER unread: FrameReader's bound on a frame
// (1.5 GiB of text + 64 KiB of header).
constexpr uint64_t kMaxFrame = (3ull << 29) + (64ull << 10);

// lbf_wire_frames_launch's d_work: one uint32 per split block (its count of
// delimiters, turned into the number of its first frame by the scan kernel).
// The stream's first byte lies up to 15 bytes into its first block.
constexpr uint64_t split_blocks(uint64_t stream_len) { return (stream_len + 15 + kSplitBlock - 1) / kSplitBlock; }
constexpr uint64_t split_work_bytes(uint64_t stream_len) { return 4 * split_blocks(stream_len); }

// lbf_wire_send_chunks_launch's d_work: one uint32 per frame (the global
// number of the chunk it is bound to, UINT32_MAX for none), then one uint32
// per kBindBlock frames (the count of bound frames, then the group's base in
// the dense tables).
constexpr uint64_t bind_blocks(uint64_t n_frames) { return (n_frames + kBindBlock - 1) / kBindBlock; }
constexpr uint64_t bind_work_bytes(uint64_t n_frames) { return 4 * n_frames + 4 * bind_blocks(n_frames); }

// The tables of one split, all device memory.
struct WireSplit {
  const uint8_t* stream;
  uint32_t stream_len;
  uint64_t* frame_off;  // null with frame_len when max_frames == 0
  uint32_t* frame_len;
  uint32_t max_frames;
  uint32_t* n_frames;
  uint64_t* tail;
  uint32_t* counts;     // split_blocks(stream_len) words of d_work
};

// The tables of the locate kernel, all device memory.
struct WireLocate {
  const uint8_t* stream;
  uint64_t stream_len;
  const uint64_t* frame_off;
  const uint32_t* frame_len;
  uint32_t n_frames;
  const uint32_t* live;  // null: n_frames is exact
  lbf_wire_frame* frames;
};

// The tables of the bind kernels behind it, all device memory.
struct WireBind {
  const uint8_t* stream;
  lbf_wire_frame* frames;
  uint32_t n_frames;
  const uint32_t* live;
  const uint8_t* file_names;  // the flood table, null with n_files == 0
  const uint32_t* file_name_off;
  const uint32_t* file_first;
  uint32_t n_files;
  const uint32_t* chunk_sizes;
  const uint8_t* chunk_expected;
  uint32_t n_chunks;
  uint64_t* text_off;         // the dense tables, null with max_chunks == 0
  uint32_t* text_len;
  uint32_t* expected_size;
  uint8_t* expected;
  uint32_t* chunk_of;
  uint32_t* frame_of;
  uint32_t max_chunks;
  uint32_t* n_located;
  uint32_t* chunk;            // n_frames words of d_work: the chunk a frame is bound to, UINT32_MAX for none
  uint32_t* counts;           // bind_blocks(n_frames) words of d_work
};

int launch_wire_split(const WireSplit& s, hipStream_t stream);
// locate and bind; then, with b.max_chunks, count, scan, scatter and the neutral entries
int launch_wire_locate(const WireLocate& w, const WireBind& b, hipStream_t stream);

}  // namespace wiref
}  // namespace lbf
