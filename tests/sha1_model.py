"""Pure-Python SHA-1 with an explicit (h, total, block) state -- TEST
INFRASTRUCTURE: the checker for resumable states (tests/test_update_cpu.py
pins it against hashlib and the oracle), above all for forged states that no
real chain of practical length reaches (tests/test_gpu_update.py).

A state is (h: list of 5 ints, total: int, block: bytes) with
len(block) == total % 64, as lbf_sha1_state keeps it.
"""
import struct

H0 = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
M = 0xFFFFFFFF


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & M


def compress(h, block):
    w = list(struct.unpack(">16I", block))
    for i in range(16, 80):
        w.append(_rotl(w[i - 3] ^ w[i - 8] ^ w[i - 14] ^ w[i - 16], 1))
    a, b, c, d, e = h
    for i in range(80):
        if i < 20:
            f, k = (b & c) | (~b & M & d), 0x5A827999
        elif i < 40:
            f, k = b ^ c ^ d, 0x6ED9EBA1
        elif i < 60:
            f, k = (b & c) | (d & (b | c)), 0x8F1BBCDC
        else:
            f, k = b ^ c ^ d, 0xCA62C1D6
        a, b, c, d, e = (_rotl(a, 5) + f + e + k + w[i]) & M, a, _rotl(b, 30), c, d
    return [(x + y) & M for x, y in zip(h, (a, b, c, d, e))]


def init():
    return list(H0), 0, b""


def update(state, data):
    h, total, block = state
    data = block + bytes(data)
    total += len(data) - len(block)
    full = len(data) // 64 * 64
    for p in range(0, full, 64):
        h = compress(h, data[p:p + 64])
    return h, total, data[full:]


def final(state):
    h, total, block = state
    pad = block + b"\x80" + bytes((55 - len(block)) % 64) + struct.pack(">Q", (total * 8) & 0xFFFFFFFFFFFFFFFF)
    for p in range(0, len(pad), 64):
        h = compress(h, pad[p:p + 64])
    return struct.pack(">5I", *h)
