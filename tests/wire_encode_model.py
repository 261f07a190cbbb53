"""The rule of the resumable base64 encode (lbf_b64_enc_state, lbf_hash.h) over
a plain tuple, for the tests of lbf_b64_encode_update_launch / _batch.  No GPU,
no pytest.

A state is (taken, carry, ncarry, layout): the bytes of the chunk encoded or
carried so far, the one or two bytes of the unfinished group, and the layout
(0 = xmlrpc++'s 73-character lines, 1 = unbroken RFC 4648 text).  With P(G) the
text position of group G, a piece of s bytes on a chain at t writes the
characters [P(t // 3), P((t + s) // 3)) of the chunk's text; a final piece also
the last group of a chunk whose size is no multiple of 3.  The characters
themselves come from `base64`, the separators from the rule; the whole texts
are compared with tests/wire_layouts.xmlrpc_text (pinned to xmlrpc++'s recorded
encoder output) and base64.b64encode in tests/test_b64_encode_cpu.py.

The kernel's geometry is restated here; tests/test_b64_encode_cpu.py reads
bitflood_amd/csrc/b64_encode_update.hpp and fails if these drift.
"""
import base64

XMLRPC, FLAT = 0, 1
LAYOUTS = {"xmlrpc": XMLRPC, "flat": FLAT}
LINE_GROUPS, LINE_BYTES, LINE_CHARS = 18, 54, 73
TILE_LINES = 112
TILE_GROUPS = TILE_LINES * LINE_GROUPS   # 2,016
TILE_BYTES = TILE_LINES * LINE_BYTES     # 6,048: "T" of the tile-edge cases
TILE_TEXT = TILE_LINES * LINE_CHARS      # 8,176 characters in lines
TILE_FLAT = TILE_GROUPS * 4              # 8,064 unbroken
MAX_CHUNK = 1 << 30
MAX_TAKEN = 1 << 61


def pos(group: int, layout: int) -> int:
    """P(G): the text position of group G."""
    return 4 * group if layout == FLAT else 4 * group + group // LINE_GROUPS


def text_length(size: int, layout: int) -> int:
    """T(n) = P(n // 3) + (4 if n % 3 else 0)."""
    return pos(size // 3, layout) + (4 if size % 3 else 0)


MAX_TEXT_CAP = text_length(MAX_CHUNK, XMLRPC)


def init(layout: int = XMLRPC):
    return (0, b"", 0, layout)


def sanitize(taken: int, carry: int, ncarry: int, layout: int):
    """What the launch makes of a record's four fields, forged or not: the count
    clamped below 2^61, ncarry taken from it, the carry masked to that, the
    layout's low bit.  Returns a model state."""
    taken = min(taken, MAX_TAKEN - 1)
    nc = taken % 3
    c = carry & ((1 << (8 * nc)) - 1)
    return (taken, c.to_bytes(4, "little")[:nc], nc, layout & 1)


def groups_text(data: bytes, first_group: int, layout: int) -> bytes:
    """The characters of len(data) // 3 whole groups that are groups first_group..
    of their chunk, each line's separator behind its 18th group."""
    n = len(data) // 3
    s = base64.b64encode(data[:3 * n])
    if layout == FLAT:
        return s
    out, k = [], 0
    while k < n:  # line by line: the groups up to the line's 18th, and the separator when that one is among them
        room = LINE_GROUPS - (first_group + k) % LINE_GROUPS
        take = min(room, n - k)
        out.append(s[4 * k:4 * (k + take)])
        if take == room:
            out.append(b" ")
        k += take
    return b"".join(out)


def update(state, piece: bytes, final: bool = False):
    """One piece.  Returns (state after, position of its new characters in the
    chunk's text, the characters, the chunk's text length when final else None)."""
    taken, carry, ncarry, layout = state
    assert ncarry == len(carry) == taken % 3
    have = carry + piece
    g0 = taken // 3
    whole = len(have) // 3 * 3
    chars = groups_text(have[:whole], g0, layout)
    rest = have[whole:]
    at = pos(g0, layout)
    if not final:
        return (taken + len(piece), rest, len(rest), layout), at, chars, None
    if rest:
        chars += base64.b64encode(rest)
    return init(layout), at, chars, at + len(chars)


def clip(at: int, chars: bytes, cap: int):
    """What of a piece's characters a slot of `cap` characters takes: (position,
    characters) as new_offsets - text_offsets / new_lens report them."""
    lo, hi = min(at, cap), min(at + len(chars), cap)
    return lo, chars[lo - at:hi - at]


def record(state):
    """A model state as the record's fields (taken, carry, ncarry, layout, zero)."""
    taken, carry, ncarry, layout = state
    return (taken, int.from_bytes(carry, "little"), ncarry, layout, 0)


def whole_text(data: bytes, layout: int) -> bytes:
    """The chunk's text in one piece, by the model."""
    return update(init(layout), data, True)[2]
