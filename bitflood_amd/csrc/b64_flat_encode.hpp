// b64_flat_encode.hpp -- what wire_batch.cpp needs of the one-shot flat encode
// (b64_flat_encode.hip): a chunk's bytes as its unbroken RFC 4648 text, the
// layout bitflood's Java and Perl peers write (LBF_B64_LAYOUT_FLAT), in one
// tiled pass; the geometry of that pass; and the layout check and the choice
// between this pass and the line kernel's, for both verify + encode calls.
// Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "b64_encode_update.hpp"
#include "lbf_hash.h"
#include "lbf_internal.hpp"

namespace lbf {

// The tile: 3 * kFlatEncTileGroups bytes -> 4 * kFlatEncTileGroups characters,
// kFlatEncTilesPerGroup consecutive tiles of a chunk per workgroup.
// tests/wire_flat_encode_model.py restates both.  2,048 groups are 512 blocks
// of 16 characters, two for every lane, and one tile per workgroup ran best:
// alternating runs of 1,024 x 256 KiB gave 98.8-101.9 us against 101.8-104.8 for
// 2,016 groups (the line kernel's tile) at one tile, 107.6-110.9 at two (the
// piecewise flat tile's shape) and 123.5-124.4 at four; 1,024, 1,536, 3,072 and
// 4,032 groups at one tile gave 109.7-110.6, 102.2-102.7, 102.6-103.3 and
// 104.0-106.2 (profiles/b64_flat_encode/ab_geometry.json).  The two macros
// exist for such A/B builds.
#ifndef LBF_B64_FLAT_ENC_TILE_GROUPS
#define LBF_B64_FLAT_ENC_TILE_GROUPS 2048
#endif
#ifndef LBF_B64_FLAT_ENC_TILES_PER_GROUP
#define LBF_B64_FLAT_ENC_TILES_PER_GROUP 1
#endif
constexpr uint32_t kFlatEncTileGroups = LBF_B64_FLAT_ENC_TILE_GROUPS;
constexpr uint32_t kFlatEncTileBytes = 3 * kFlatEncTileGroups;  // 6,144 bytes
constexpr uint32_t kFlatEncTileText = 4 * kFlatEncTileGroups;   // 8,192 characters
constexpr uint32_t kFlatEncTilesPerGroup = LBF_B64_FLAT_ENC_TILES_PER_GROUP;

// n chunks' bytes -> their unbroken text, on `stream`: chunk i =
// data[data_off[i], + size[i]) -> text[text_off[i], + 4 * ceil(size[i] / 3)).
// max_size (at most b64e::kEncMaxChunk) sets the tiles per chunk: a larger chunk's
// text stays incomplete, and nothing outside its slot is written.
int launch_b64_flat_encode(const uint8_t* data, const uint64_t* data_off, const uint32_t* size, uint8_t* text,
                           const uint64_t* text_off, uint32_t n, uint32_t max_size, hipStream_t stream);

// The verify + encode calls' first refusal: a layout that is neither peer's.
inline int check_b64_layout(const std::string& who, int layout) {
  if (layout != LBF_B64_LAYOUT_XMLRPC && layout != LBF_B64_LAYOUT_FLAT)
    return fail(LBF_ERR_INVALID, who + ": layout is neither LBF_B64_LAYOUT_XMLRPC nor LBF_B64_LAYOUT_FLAT");
  return LBF_OK;
}

// The layout's one-shot encode: this file's pass, or the line kernel's (kern_b64.hpp).
inline int launch_b64_encode_for(int layout, const uint8_t* data, const uint64_t* data_off, const uint32_t* size,
                                 uint8_t* text, const uint64_t* text_off, uint32_t n, uint32_t max_size,
                                 hipStream_t stream) {
  return layout == LBF_B64_LAYOUT_FLAT
             ? launch_b64_flat_encode(data, data_off, size, text, text_off, n, max_size, stream)
             : launch_b64_encode(data, data_off, size, text, text_off, n, max_size, stream);
}

}  // namespace lbf
