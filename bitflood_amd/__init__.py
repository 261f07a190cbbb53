"""bitflood_amd -- MI355X-native chunk-hash path for bitflood.

Product pieces:
  bitflood_amd/csrc/      HIP kernels (gfx950) + C ABI  -> bitflood_amd/lib/liblbfhash.so
  bitflood_amd/host/      C++ libBitFlood layer (Encoder / FloodFile / verify) -> libbitflood.so
  include/                the public headers of both
  bitflood_amd/hashing.py Python binding used by tests and bench.py

See DESIGN.md for the path, the boundary and the kernels.
"""
from . import _capi  # noqa: F401  (imports torch first: one HIP runtime per process)
from .hashing import (B64_ENC_STATE_DTYPE, B64_STATE_DTYPE, STATE_DTYPE, ChunkHasher, DeviceBuffer,  # noqa: F401
                      LbfError, b64_27, b64_27_decode, b64_encode_update_launch, b64_text_length, b64_update_launch,
                      b64_update_seq_launch, b64_verify_launch_work, chain_table, chunk_table, new_b64_enc_states, new_b64_states,
                      new_states, set_b64_flat, set_b64_fused, set_b64_lines, sha1_hashes_launch, update_seq_launch,
                      verify_b64_launch, verify_encode_b64_launch, verify_hashes_launch, verify_hashes_launch_work)
from .hashing import (LBF_FRAME_OTHER, LBF_FRAME_SEND_CHUNK, LBF_FRAME_SEND_CHUNK_UNBOUND,  # noqa: F401
                      WIRE_FRAME_DTYPE, wire_flood_table, wire_frames_launch, wire_frames_launch_work,
                      wire_send_chunks_launch, wire_send_chunks_launch_work, xml_encode)

__version__ = "0.1.0"
