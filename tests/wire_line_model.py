"""The line path of the piecewise base64 decode (bitflood_amd/csrc/
b64_update_lines.hip), restated -- TEST INFRASTRUCTURE: which prefix of a piece
continues xmlrpc++'s layout from where the record stands, and what it decodes
to when every character is read from its known place.  No GPU, no pytest.

tests/test_b64_lines_cpu.py holds it against tests/wire_piece_model.update
(pinned to xmlrpc++'s recorded answers): on the prefix `take` returns, the
places' decode and the general rule give the same bytes and the same state.

The rule.  A state that has not ended and has decoded a multiple of 3 bytes
has taken S = 4 * decoded / 3 + ncarry sextets, so the piece's first character
stands at column S mod 72 of a line of 72 alphabet characters and a separator:
  - at column 0 one leading character outside the alphabet and other than '='
    is the separator, whether S is 0 or not;
  - a carried group is completed from the next 4 - ncarry characters, all of
    the alphabet;
  - whole groups of four alphabet characters follow; a group that ends a line
    is followed by one character outside the alphabet (and not '='), which is
    taken, or by the end of the piece;
  - the prefix ends behind a group (nothing is carried) or behind a
    separator, and in front of any '='.
The kernel may take less (it gives up a whole tile that breaks the layout),
never more.
"""
import numpy as np

from tests.wire_piece_model import EQ, SKIP, TABLE

LINE = 72  # alphabet characters to a line


def _bytes(c):
    return bytes([((c[0] << 2) | (c[1] >> 4)) & 255, ((c[1] << 4) | (c[2] >> 2)) & 255, ((c[2] << 6) | c[3]) & 255])


def take(state, piece: bytes):
    """(characters taken, the bytes they decode to by their places, the state
    after them) for the longest prefix of `piece` the line path may take."""
    decoded, carry, ended = state
    n = len(piece)
    if ended or decoded % 3 != 0 or n == 0:
        return 0, b"", state
    v = TABLE[np.frombuffer(bytes(piece), dtype=np.uint8)]
    col = (4 * decoded // 3 + len(carry)) % LINE
    pos, head = 0, b""
    if col == 0 and v[0] == SKIP:
        pos = 1
    if carry:
        need = 4 - len(carry)
        if n < need or (v[:need] >= EQ).any():
            return 0, b"", state
        head = _bytes(list(carry) + [int(x) for x in v[:need]])
        pos, col = need, col + need
    # character k >= pos stands at place (col + k - pos) mod 73 of its line: 0..71 a group's, 72 the separator's
    place = (col + np.arange(n - pos)) % (LINE + 1)
    fits = np.where(place == LINE, v[pos:] == SKIP, v[pos:] < EQ)
    run = int(np.flatnonzero(~fits)[0]) if not fits.all() else n - pos
    # the prefix ends behind a group or a separator: the next place is a multiple of 4
    while (col + run) % (LINE + 1) % 4 != 0:
        run -= 1
    s = v[pos:pos + run][place[:run] != LINE].astype(np.uint32).reshape(-1, 4)
    w = (s[:, 0] << 18) | (s[:, 1] << 12) | (s[:, 2] << 6) | s[:, 3]
    out = np.empty((len(s), 3), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = w >> 16, (w >> 8) & 255, w & 255
    body = head + out.tobytes()
    return pos + run, body, (decoded + len(body), (), False)
