"""xmlrpc++ 0.7's base64 decoder (base64.h:215-330) stopped between pieces --
TEST INFRASTRUCTURE: the checker for lbf_b64_state (include/lbf_hash.h) after
a piece that is not the last.  No GPU, no pytest.

tests/test_b64_update_cpu.py pins it to the decoder's recorded answers
(tests/golden/xmlrpc07_base64_get.json) at every cutting of the recorded
texts, and to tests/wire_layouts.b64get on every tiny text at every cut.

A state is (decoded: int, carry: tuple of pending sextets, ended: bool).
"""
import numpy as np

from tests import sha1_model
from tests.wire_layouts import ALPHABET, EQ, SKIP

# the decoder's table: a sextet, EQ for '=', SKIP for every other character
TABLE = np.full(256, SKIP, dtype=np.int16)
TABLE[np.frombuffer(ALPHABET, dtype=np.uint8)] = np.arange(64)
TABLE[ord("=")] = EQ


def init():
    return 0, (), False


def update_by_character(state, text: bytes):
    """Feed one piece; returns (state, the bytes it newly decodes)."""
    decoded, carry, ended = state
    if ended:
        return state, b""
    c = list(carry)
    out = bytearray()
    for ch in bytes(text):
        v = int(TABLE[ch])
        if v == SKIP:
            continue
        if v == EQ:  # the first '=' ends the data: one more byte with 2 sextets pending, two with 3
            if len(c) >= 2:
                out.append(((c[0] << 2) | (c[1] >> 4)) & 255)
            if len(c) == 3:
                out.append(((c[1] << 4) | (c[2] >> 2)) & 255)
            return (decoded + len(out), (), True), bytes(out)
        c.append(v)
        if len(c) == 4:
            out += bytes([((c[0] << 2) | (c[1] >> 4)) & 255, ((c[1] << 4) | (c[2] >> 2)) & 255,
                          ((c[2] << 6) | c[3]) & 255])
            c = []
    return (decoded + len(out), tuple(c), False), bytes(out)


def update(state, text: bytes):
    """update_by_character's rule without its loop (tests/test_b64_update_cpu.py
    holds the two together): S = the pending sextets, then the piece's
    characters of the alphabet and '='; q = the index of the first '=' in S
    (len(S) if none); the complete groups before q give three bytes each, a
    '=' one more with q % 4 == 2 and two with 3, and without '=' the q % 4
    sextets left are carried."""
    decoded, carry, ended = state
    if ended:
        return state, b""
    v = TABLE[np.frombuffer(bytes(text), dtype=np.uint8)]
    s = np.concatenate([np.array(carry, dtype=np.uint32), v[v != SKIP].astype(np.uint32)])
    eq = np.flatnonzero(s == EQ)
    q = int(eq[0]) if eq.size else s.size
    g = q // 4
    x = s[:4 * g].reshape(g, 4)
    w = (x[:, 0] << 18) | (x[:, 1] << 12) | (x[:, 2] << 6) | x[:, 3]
    out = np.empty((g, 3), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = w >> 16, (w >> 8) & 255, w & 255
    rest = [int(k) for k in s[4 * g:q]]
    if not eq.size:
        return (decoded + 3 * g, tuple(rest), False), out.tobytes()
    tail = b""
    if len(rest) >= 2:
        tail = bytes([((rest[0] << 2) | (rest[1] >> 4)) & 255])
    if len(rest) == 3:
        tail += bytes([((rest[1] << 4) | (rest[2] >> 2)) & 255])
    return (decoded + 3 * g + len(tail), (), True), out.tobytes() + tail


def final(state) -> int:
    """The last piece is in: an unfinished group is dropped.  The decoded length."""
    return state[0]


def decode_pieces(pieces, step=None) -> bytes:
    st, out = init(), b""
    for p in pieces:
        st, b = (step or update)(st, p)
        out += b
    return out


def b64_record(state):
    """The state as a lbf_b64_state: (decoded, carry, ncarry, ended, zero)."""
    decoded, carry, ended = state
    return decoded, sum(v << (6 * k) for k, v in enumerate(carry)), len(carry), int(ended), 0


def b64_records(states, dtype) -> np.ndarray:
    return np.array([b64_record(s) for s in states], dtype=dtype)


_H = {b"": list(sha1_model.H0)}  # chaining value after each prefix of whole blocks seen so far


def sha_state(prefix: bytes, cap: int):
    """sha1_model's state of the partner chain: it has absorbed what lies below
    cap.  Chains of one test share prefixes, so the chaining values are kept."""
    data = bytes(prefix[:cap])
    full = len(data) // 64 * 64
    k = full
    while data[:k] not in _H:
        k -= 64
    h = _H[data[:k]]
    for p in range(k, full, 64):
        h = sha1_model.compress(h, data[p:p + 64])
        _H[data[:p + 64]] = h
    return list(h), len(data), data[full:]


def sha_records(states, dtype) -> np.ndarray:
    """sha1_model states as lbf_sha1_state records (block bytes past `buffered` zero)."""
    rec = np.zeros(len(states), dtype=dtype)
    for k, (h, total, block) in enumerate(states):
        rec["h"][k], rec["total"][k], rec["buffered"][k] = h, total, len(block)
        rec["block"][k, :len(block)] = np.frombuffer(block, dtype=np.uint8)
    return rec


def sha_records_differ(got: np.ndarray, want: np.ndarray):
    """Indices where two arrays of lbf_sha1_state differ, the block's bytes past `buffered` left out."""
    live = np.arange(64)[None, :] < want["buffered"][:, None]
    bad = ((got["h"] != want["h"]).any(axis=1) | (got["total"] != want["total"]) | (got["buffered"] != want["buffered"])
           | ((got["block"] != want["block"]) & live).any(axis=1))
    return np.flatnonzero(bad).tolist()
