"""The wire (base64) kernels of bitflood_amd/csrc/kern_b64.hpp past their first
tile and at every damage position.

tests/test_gpu_b64.py damages texts at random places of their first tile.
Here the damage is placed by structure (tests/wire_layouts.py; what each
corpus reaches is proven on the CPU by tests/test_wire_layouts.py): every
character of a period of the line / block / lane grids, both sides of tile,
workgroup and scan-trip edges, slots and texts that disagree by whole tiles,
the general decode's carries across scan trips, a batch past one launch slice,
and the encode's tile edges at every source phase.

Every decode case is held to the same five assertions (`_decode_and_check`):
the expected bytes come from wire_layouts.decode alone (pinned to xmlrpc++'s
own decoder by tests/golden/xmlrpc07_base64_get.json); `out` is 0x5A with gaps
of 0..20 bytes between the slots; a call before it leaves 0xEE and other
non-zero bytes all over the device scratch; then
  - each slot is the decoded bytes cut to the slot, then zeros,
  - the reported length is the decoded length, or the slot's size + 1 when longer,
  - the verdict is 1 exactly when the decoded bytes are the chunk,
  - every byte outside the slots is still 0x5A,
  - the b64_stats deltas are the counts of texts inside and outside the
    encoder's layout (wire_layouts.is_encoder_layout).
"""
import hashlib

import numpy as np
import pytest

from tests import wire_layouts as W

pytestmark = pytest.mark.gpu

FILL = 0x5A


def _digests(corpus):
    exp = np.frombuffer(b"".join(hashlib.sha1(d).digest() for d in corpus.chunks), dtype=np.uint8)
    exp = exp.reshape(-1, 20).copy()
    wrong = np.flatnonzero(~np.array(corpus.digest_ok, dtype=bool))
    exp[wrong, 0] ^= 1
    return exp


def _leave_stale_bytes(hasher, nbytes):
    """One 0xEE-filled chunk larger than the batch that follows: its text, its
    sextets and its bytes lie where the batch's decoded bytes will."""
    d = b"\xEE" * nbytes
    ver, dec = hasher.verify_b64(np.frombuffer(W.filler_text(nbytes), np.uint8), [0], [W.b64_len(nbytes)], [nbytes],
                                 np.frombuffer(hashlib.sha1(d).digest(), np.uint8).reshape(1, 20))
    assert ver.all() and int(dec[0]) == nbytes


def _gap_here(i, gap_every):
    """Whether slot i gets a gap in front: every slot, or (a batch of tens of
    thousands of small slots, whose results come back one copy per run of
    touching slots) every gap_every-th and each one around the launch slice."""
    return i % gap_every == 0 or abs(i - W.CHUNKS_PER_LAUNCH) < 40


def _encode(hasher, data, offs, sizes, exp, tslot, tbuf):
    """lbf_verify_encode_b64_batch through the raw C call: the caller lays out the text slots."""
    n = len(sizes)
    ver = np.zeros(n, dtype=np.uint8)
    rc = hasher._lib.lbf_verify_encode_b64_batch(hasher._h, data.ctypes.data, data.size, offs.ctypes.data,
                                                 sizes.ctypes.data, n, exp.ctypes.data, ver.ctypes.data,
                                                 tbuf.ctypes.data, tbuf.size, tslot.ctypes.data)
    assert rc == 0, hasher._lib.lbf_last_error()
    return ver.astype(bool)


def _check_texts(tbuf, tslot, texts, what):
    """Every slot holds its text and every other byte of tbuf is still 0xCD."""
    want = bytearray(b"\xCD" * tbuf.size)
    for o, t in zip(tslot, texts):
        want[int(o):int(o) + len(t)] = t
    want = np.frombuffer(bytes(want), dtype=np.uint8)
    bad = np.flatnonzero(tbuf != want)
    if bad.size:
        b = int(bad[0])
        i = max(int(np.searchsorted(tslot, b, side="right")) - 1, 0)
        pytest.fail(f"{bad.size} characters differ; the first is text byte {b}, {b - int(tslot[i])} from the slot of "
                    f"{what(i)}: got {tbuf[b]:#04x}, want {want[b]:#04x}")


def _decode_and_check(hasher, c, gap_every=1):
    n = len(c)
    # the texts, at their phases mod 16, between characters a decode must not read as the chunk's
    pieces, toff, pos = [], np.zeros(n, dtype=np.uint64), 0
    for i, t in enumerate(c.texts):
        gap = i % 3 if c.tphase[i] is None else (c.tphase[i] - pos) % 16
        pieces.append((b"A=" * 8)[:gap])
        pos += gap
        toff[i] = pos
        pieces.append(t)
        pos += len(t)
    pieces.append(b"A=")
    text = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    tlen = np.array([len(t) for t in c.texts], dtype=np.uint32)
    # the slots: 0..20 bytes of gap in front of each
    caps = np.array(c.caps, dtype=np.uint32)
    ooff, pos = np.zeros(n, dtype=np.uint64), 0
    for i in range(n):
        if c.sphase[i] is not None:
            pos += (c.sphase[i] - pos) % 16
        elif _gap_here(i, gap_every):
            pos += 7 * i % 21
        ooff[i] = pos
        pos += int(caps[i])
    out = np.full(pos + 13, FILL, dtype=np.uint8)
    expected = c.expected()
    want = bytearray(bytes([FILL]) * out.size)
    for i, (w, _, _) in enumerate(expected):
        cap, o = int(caps[i]), int(ooff[i])
        want[o:o + cap] = w[:cap].ljust(cap, b"\0")
    want = np.frombuffer(bytes(want), dtype=np.uint8)
    exp = _digests(c)
    sext = int(((tlen.astype(np.int64) + 15) // 16 * 16).sum())
    _leave_stale_bytes(hasher, max(out.size, (text.size + sext + out.size) // 3) + 4096)
    s0 = hasher.b64_stats()
    ver, dec = hasher.verify_b64(text, toff, tlen, caps, exp, out, ooff)
    s1 = hasher.b64_stats()

    def entry_of(byte):
        i = int(np.searchsorted(ooff, byte, side="right")) - 1
        while i > 0 and caps[i] == 0 and byte >= int(ooff[i]) + int(caps[i]):
            i -= 1  # an empty slot owns nothing
        i = max(i, 0)
        inside = int(ooff[i]) <= byte < int(ooff[i]) + int(caps[i])
        place = f"byte {byte - int(ooff[i])} of the slot of " if inside else "a byte outside the slots, behind "
        return place + c.desc[i]

    bad = np.flatnonzero(out != want)
    if bad.size:
        b = int(bad[0])
        pytest.fail(f"{bad.size} bytes differ; the first is {entry_of(b)}: got {out[b]:#04x}, want {want[b]:#04x}")
    want_len = np.array([e[1] for e in expected], dtype=np.int64)
    bad = np.flatnonzero(dec.astype(np.int64) != want_len)
    assert bad.size == 0, (c.desc[int(bad[0])], int(dec[bad[0]]), int(want_len[bad[0]]), bad.size)
    want_ver = np.array([e[2] for e in expected], dtype=bool)
    bad = np.flatnonzero(ver != want_ver)
    assert bad.size == 0, (c.desc[int(bad[0])], bool(ver[bad[0]]), bad.size)
    one, general = c.layout_counts()
    assert (s1["one_pass"] - s0["one_pass"], s1["general"] - s0["general"]) == (one, general)
    return ver, dec, want_ver


@pytest.mark.parametrize("kind", W.KINDS)
def test_every_position_of_a_period(hasher, kind):
    """Test 1: `kind` at every character of 16-line texts: every column of a
    line at every phase of the one-pass decode's blocks and at every byte of
    the general decode's lanes, separators and the padded last group included."""
    _decode_and_check(hasher, W.period_corpus(kind))


@pytest.mark.parametrize("kind", W.KINDS)
def test_tile_and_workgroup_edges(hasher, kind):
    """Test 2: `kind` on both sides of the one-pass decode's tile and workgroup
    edges, of the general decode's scan trips 1, 2 and 6, and in the last 80
    characters, of 28 KB texts (five tiles and a part, seven trips)."""
    _decode_and_check(hasher, W.edge_corpus(kind))


def test_slot_and_text_lengths_disagree(hasher):
    """Test 3: a frame cut short or too long for its slot, by bytes, by whole
    tiles and by a whole workgroup, on both decode paths: the slot's rest is
    zeroed, nothing outside it is written, the length says which way."""
    c = W.disagree_corpus()
    ver, dec, _ = _decode_and_check(hasher, c)
    assert not ver.any()


def test_general_decode_across_scan_trips(hasher):
    """Test 4: what the general decode carries from one scan trip to the next:
    the count of valid characters (lanes holding 0..16 of them, whole trips
    holding none), the first '=' (on both sides of a trip at every q % 4, and
    two in one trip), and the last partial trip of either pass."""
    c = W.scan_corpus()
    ver, dec, want_ver = _decode_and_check(hasher, c)
    assert want_ver.any() and not want_ver.all()


def test_more_chunks_than_one_launch_slice(hasher):
    """Test 5: 65,535 + 300 chunks: the tiled launches take the batch in slices
    of 65,535 and tell the kernel where its slice starts, for the decode and
    for the encode.  Most of these small slots touch their neighbours (every
    run of touching slots is one copy back; 65,835 copies took 2 s), with a
    gap in front of every 16th and of each of the 80 around the slice edge."""
    c = W.slices_corpus()
    n = len(c)
    ver, dec, want_ver = _decode_and_check(hasher, c, gap_every=16)
    assert want_ver[W.CHUNKS_PER_LAUNCH:].any() and not want_ver[W.CHUNKS_PER_LAUNCH:].all()
    sizes = np.array([len(d) for d in c.chunks], dtype=np.uint32)
    offs = np.concatenate(([0], np.cumsum(sizes[:-1], dtype=np.uint64))).astype(np.uint64)
    data = np.frombuffer(b"".join(c.chunks), dtype=np.uint8)
    texts = [W.xmlrpc_text(d) for d in c.chunks]
    tslot, pos = np.zeros(n, dtype=np.uint64), 0
    for i, t in enumerate(texts):  # touching text slots at every phase, a sentinel gap here and there
        if _gap_here(i, 16):
            pos += 1 + 7 * i % 21
        tslot[i] = pos
        pos += len(t)
    tbuf = np.full(pos + 21, 0xCD, dtype=np.uint8)
    ver = _encode(hasher, data, offs, sizes, _digests(c), tslot, tbuf)
    _check_texts(tbuf, tslot, texts, lambda i: f"chunk {i} ({sizes[i]} B)")
    bad = np.flatnonzero(ver != np.array(c.digest_ok, dtype=bool))
    assert bad.size == 0, (int(bad[0]), bad.size)


def test_encode_tile_edges_at_every_source_phase(hasher):
    """Test 6: chunk sizes on both sides of the encode's tile, workgroup and
    line edges, sources at every phase mod 16 (the staging's `delta`), text
    slots at 0, 1, 8 and 15 mod 16 in a 0xCD buffer; then the texts, where
    they lie, back through the decode."""
    cases = W.encode_cases()
    n = len(cases)
    rng = np.random.default_rng(66)
    offs, tslot, dpos, tpos = np.zeros(n, np.uint64), np.zeros(n, np.uint64), 0, 0
    for i, (size, sphase, tphase) in enumerate(cases):
        dpos += (sphase - dpos) % 16
        offs[i] = dpos
        dpos += size
        tpos += 1 + (tphase - tpos - 1) % 16  # at least one sentinel byte between slots
        tslot[i] = tpos
        tpos += W.b64_len(size)
    data = rng.integers(0, 256, dpos + 16, dtype=np.uint8)
    sizes = np.array([s for s, _, _ in cases], dtype=np.uint32)
    datas = [data[int(o):int(o) + int(s)].tobytes() for o, s in zip(offs, sizes)]
    assert [int(o) % 16 for o in offs] == [p for _, p, _ in cases]
    assert [int(o) % 16 for o in tslot] == [p for _, _, p in cases]
    exp = np.frombuffer(b"".join(hashlib.sha1(d).digest() for d in datas), dtype=np.uint8).reshape(-1, 20).copy()
    exp[::5, 19] ^= 0x80
    tbuf = np.full(tpos + 33, 0xCD, dtype=np.uint8)
    ver = _encode(hasher, data, offs, sizes, exp, tslot, tbuf)
    texts = [W.xmlrpc_text(d) for d in datas]
    _check_texts(tbuf, tslot, texts, lambda i: f"case {i} {cases[i]}")
    assert [bool(v) for v in ver] == [i % 5 != 0 for i in range(n)]
    # the round trip: the device's own texts through the decode, at the phases they were written at
    c = W.Corpus("encode round trip")
    for i, d in enumerate(datas):
        t = tbuf[int(tslot[i]):int(tslot[i]) + len(texts[i])].tobytes()
        c.add(t, d, f"case {i} {cases[i]}", tphase=cases[i][2])
    ver, dec, _ = _decode_and_check(hasher, c)
    assert ver.all()
