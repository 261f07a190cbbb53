"""The flat path of the base64 decode (bitflood_amd/csrc/b64_flat.hip),
restated -- TEST INFRASTRUCTURE: which chunks the one-shot flat pass decodes,
and which part of a piece the piecewise flat kernel takes and what that decodes
to when character i is sextet i.  No GPU, no pytest.

The layout.  bitflood's Java and Perl peers frame a chunk as unbroken RFC 4648
text: 4 * ceil(size / 3) characters, '=' padding, no line separators.  Neither
peer can be run where these tests run, so the layout rests on three
source lines of the reference: java/com/net/BitFlood/XMLEnvelopeProcessor.java:124
(Base64.encodeToString(arg, false): sdk/Base64.java with lineSep == false) and
perl/RPC/XML.pm:638 (MIME::Base64::encode_base64($value, ''), and :671, :734
for file-backed values).  `text` below is that layout: base64.b64encode.

tests/test_b64_flat_cpu.py holds the model against tests/wire_piece_model.update
and tests/wire_layouts.decode (both pinned to xmlrpc++'s recorded answers).

One-shot.  A chunk is a candidate when its text's length is the unbroken
text's and not the encoder's, and the chunk is larger than 54 bytes (up to 53
the two layouts are one text, and the 72 characters of 54 bytes are a line that
the one-pass decode takes without its trailing separator: those stay with it).
A candidate is decoded flat when every character is of the alphabet, except
that the last group may be "xx==" or "xxx="; any other candidate goes to the
general decode.

Piecewise.  From a state that has not ended and has decoded a multiple of 3
bytes, of the characters the line path left:
  - a carried group is completed from the next 4 - ncarry characters, all of
    the alphabet;
  - whole groups of four alphabet characters follow, up to the last whole
    group of the remainder, or the one before it when that one holds '=';
  - the prefix ends behind a group, so nothing is carried.
`take` gives the longest such prefix.  The kernel validates by tiles of 1,296
groups laid over the chunk (tile k holds chunk bytes [3888k, +3888)): a tile
with a character outside the alphabet among the groups it was given takes
nothing and ends the prefix at its start; `take(..., tiles=True)` is that.
"""
import base64

import numpy as np

from tests.wire_layouts import b64_len
from tests.wire_piece_model import EQ, TABLE

TILE_BYTES = 3888
TILE_GROUPS, TILE_TEXT = TILE_BYTES // 3, TILE_BYTES // 3 * 4  # 1,296 / 5,184


def text(data: bytes) -> bytes:
    """A chunk as a Java or Perl peer frames it."""
    return base64.b64encode(data)


def flat_len(size: int) -> int:
    return 4 * ((size + 2) // 3)


def is_candidate(text_len: int, expected_size: int) -> bool:
    return expected_size > 54 and text_len == flat_len(expected_size) and text_len != b64_len(expected_size)


def is_flat(t: bytes) -> bool:
    """Whole groups of the alphabet; the last may be "xx==" or "xxx="."""
    if len(t) % 4 or not t:
        return False
    v = TABLE[np.frombuffer(bytes(t), dtype=np.uint8)]
    if (v[:-2] >= EQ).any():
        return False
    c2, c3 = int(v[-2]), int(v[-1])
    return (c2 < EQ and c3 < EQ) or (c2 < EQ and c3 == EQ) or (c2 == EQ and c3 == EQ)


def decoded_flat(t: bytes, expected_size: int) -> bool:
    """Whether the one-shot flat pass keeps this chunk."""
    return is_candidate(len(t), expected_size) and is_flat(t)


def _bytes_of(v) -> bytes:
    s = v.astype(np.uint32).reshape(-1, 4)
    w = (s[:, 0] << 18) | (s[:, 1] << 12) | (s[:, 2] << 6) | s[:, 3]
    out = np.empty((len(s), 3), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = w >> 16, (w >> 8) & 255, w & 255
    return out.tobytes()


def take(state, rest: bytes, tiles: bool = False):
    """(characters taken, the bytes they decode to by their places, the state
    after them) for the prefix of `rest` the flat path takes."""
    decoded, carry, ended = state
    n = len(rest)
    if ended or decoded % 3 != 0 or n == 0:
        return 0, b"", state
    v = TABLE[np.frombuffer(bytes(rest), dtype=np.uint8)]
    pos, head = 0, b""
    if carry:
        need = 4 - len(carry)
        if n < need or (v[:need] >= EQ).any():
            return 0, b"", state
        head = _bytes_of(np.array(list(carry) + [int(x) for x in v[:need]]))
        pos = need
    groups = (n - pos) // 4
    if groups and (v[pos + 4 * (groups - 1):pos + 4 * groups] == EQ).any():
        groups -= 1
    ok = (v[pos:pos + 4 * groups].reshape(-1, 4) < EQ).all(axis=1)  # per group
    if not tiles:
        good = int(np.flatnonzero(~ok)[0]) if not ok.all() else groups
    else:
        # group k of the prefix is group g_first + k of the chunk's tile grid
        g_first = (decoded + len(head)) // 3 % TILE_GROUPS
        good = 0
        while good < groups:
            end = min(groups, (g_first + good) // TILE_GROUPS * TILE_GROUPS + TILE_GROUPS - g_first)
            if not ok[good:end].all():
                break
            good = end
    if pos + good == 0:
        return 0, b"", state
    body = head + _bytes_of(v[pos:pos + 4 * good])
    return pos + 4 * good, body, (decoded + len(body), (), False)


def most_behind_lines(rest_from: int, piece: bytes) -> int:
    """An upper bound on what the flat kernel takes of `piece` when the line
    path ran in front and stopped somewhere in [0, rest_from]: the flat prefix
    is consecutive alphabet characters, so no longer than the longest run of
    them that starts at or before rest_from."""
    v = TABLE[np.frombuffer(bytes(piece), dtype=np.uint8)]
    stops = np.flatnonzero(v >= EQ)
    starts = np.concatenate(([0], stops[stops + 1 <= rest_from] + 1))
    ends = np.concatenate((stops, [len(piece)]))
    nxt = ends[np.searchsorted(ends, starts)]
    return int((nxt - starts).max())
