"""CPU model of lbf_wire_frames_launch and lbf_wire_send_chunks_launch (test
infrastructure, no test of its own): the '\\n' split, a restatement of
PeerWire::LocateSendChunk (bitflood_amd/host/PeerWire.cpp) that returns raw
ranges, the binding against a flood table, and frame builders that restate
EncodeSendChunk / EncodeMethod.  tests/test_wire_frames_cpu.py pins locate(),
xml_decode() and the builders against the C++ itself."""
import base64
import hashlib
import re

import numpy as np

SPACE = b" \t\n\v\f\r"  # isspace() of the C locale
OTHER, SEND_CHUNK, UNBOUND = 0, 1, 2
MAX_FRAME = (3 << 29) + (64 << 10)
NONE = 0xFFFFFFFF
REQUEST_BEGIN = b'<?xml version="1.0"?>\r\n<methodCall><methodName>'
REQUEST_END_NAME = b"</methodName>\r\n"
REQUEST_END = b"</methodCall>\r\n"
_ENT = ((b"<", b"&lt;"), (b">", b"&gt;"), (b"&", b"&amp;"), (b"'", b"&apos;"), (b'"', b"&quot;"))


# ---- the split -------------------------------------------------------------
def split(stream: bytes):
    """([(offset, length)], tail): the frames the delimiters end, and where the unfinished one starts."""
    frames, start = [], 0
    while True:
        p = stream.find(b"\n", start)
        if p < 0:
            return frames, start
        frames.append((start, p - start))
        start = p + 1


# ---- LocateSendChunk -------------------------------------------------------
def _find(s, frm, needle):
    if frm >= len(s) or len(needle) > len(s) - frm:
        return -1
    return s.find(needle, frm)


def _skip(s, p):
    while p < len(s) and s[p] in SPACE:
        p += 1
    return p


def _next_tag_is(tag, s, off):
    """off behind the tag, or None."""
    p = _skip(s, off)
    return p + len(tag) if s[p:p + len(tag)] == tag else None


def _get_next_tag(s, off):
    p = _skip(s, off)
    if p >= len(s) or s[p] != 0x3C:
        return b"", off
    g = s.find(b">", p)
    e = len(s) if g < 0 else g + 1
    return s[p:e], e


def strtol_u32(tok: bytes):
    """(U32)(int)strtol(tok, &end, 10) and end - tok, or None when no digit stands there."""
    tok = tok.split(b"\0")[0]
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?)([0-9]+)", tok)
    if not m:
        return None
    x = int(m.group(2)) * (-1 if m.group(1) == b"-" else 1)
    x = max(-(1 << 63), min((1 << 63) - 1, x))
    return x & 0xFFFFFFFF, m.end()


def _parse_value(s, off):
    """(kind, payload, off) with kind in 'str' 'int' 'bin', or None."""
    off = _next_tag_is(b"<value>", s, off)
    if off is None:
        return None
    after_value = off
    tag, off = _get_next_tag(s, off)
    if tag in (b"<i4>", b"<int>"):
        ws = _skip(s, off)
        got = strtol_u32(s[ws:ws + 63])
        if got is None:
            return None
        off = _next_tag_is(b"</i4>" if tag == b"<i4>" else b"</int>", s, ws + got[1])
        if off is None:
            return None
        kind, payload = "int", got[0]
    elif tag in (b"", b"<string>", b"</value>"):
        if tag == b"</value>":
            off = after_value
        lt = s.find(b"<", off)
        if lt < 0:
            return None
        kind, payload, off = "str", (off, lt - off), lt
    elif tag == b"<base64>":
        lt = s.find(b"<", off)
        if lt < 0:
            return None
        kind, payload, off = "bin", (off, lt - off), lt
    else:
        return None
    e = _find(s, off, b"</value>")
    return kind, payload, (e + 8 if e >= 0 else off)


def locate(frame: bytes):
    """None, or dict(name_off, name_len, index, text_off, text_len) as positions in the frame."""
    s = bytes(frame)
    a = _find(s, 0, b"<methodName>")
    if a < 0:
        return None
    b = a + 12
    e = _find(s, b, b"</methodName>")
    if e < 0 or s[b:e] != b"SendChunk":
        return None
    pp = _find(s, e + 13, b"<params>")
    if pp < 0:
        return None
    off = pp + 8
    out = {}
    for want in ("str", "int"):
        off = _next_tag_is(b"<param>", s, off)
        if off is None:
            return None
        v = _parse_value(s, off)
        if v is None or v[0] != want:
            return None
        if want == "str":
            out["name_off"], out["name_len"] = v[1]
        else:
            out["index"] = v[1]
        off = v[2]
        nxt = _next_tag_is(b"</param>", s, off)
        off = off if nxt is None else nxt
    for tag in (b"<param>", b"<value>"):
        off = _next_tag_is(tag, s, off)
        if off is None:
            return None
    tag, off = _get_next_tag(s, off)
    if tag != b"<base64>":
        return None
    lt = s.find(b"<", off)
    if lt < 0:
        return None
    out["text_off"], out["text_len"] = off, lt - off
    return out


# ---- names -----------------------------------------------------------------
def xml_encode(raw: bytes) -> bytes:
    out = bytearray()
    for c in raw:
        for r, e in _ENT:
            if c == r[0]:
                out += e
                break
        else:
            out.append(c)
    return bytes(out)


def xml_decode(enc: bytes) -> bytes:
    out, i = bytearray(), 0
    while i < len(enc):
        if enc[i] == 0x26:
            for r, e in _ENT:
                if enc[i:i + len(e)] == e:
                    out += r
                    i += len(e)
                    break
            else:
                out.append(enc[i])
                i += 1
        else:
            out.append(enc[i])
            i += 1
    return bytes(out)


# ---- the flood table and the binding ---------------------------------------
def flood_table(files):
    """[(name bytes, [size], [digest])] in flood order -> (names, name_off, first, sizes, digests) as lists."""
    names, name_off, first, sizes, digests = [], [0], [0], [], []
    for name, fs, fd in files:
        names.append(xml_encode(name))
        name_off.append(name_off[-1] + len(names[-1]))
        first.append(first[-1] + len(fs))
        sizes += list(fs)
        digests += [bytes(d) for d in fd]
    return names, name_off, first, sizes, digests


def bind(raw_name: bytes, index: int, table):
    """The global chunk number, or None."""
    if table is None:
        return None
    names, _, first, sizes, _ = table
    for f, n in enumerate(names):
        if n == raw_name:
            if index < first[f + 1] - first[f] and first[f] + index < len(sizes):
                return first[f] + index
            return None
    return None


def frames_expected(stream: bytes, frame_table, table, frame_dtype):
    """d_frames as the launch writes it for the live frames frame_table = [(offset, length)], and the chunk of each."""
    out = np.zeros(len(frame_table), frame_dtype)
    chunks = []
    for i, (at, n) in enumerate(frame_table):
        loc = locate(stream[at:at + n]) if n <= MAX_FRAME and at + n <= len(stream) else None
        chunk = None
        if loc is not None:
            chunk = bind(stream[at + loc["name_off"]:at + loc["name_off"] + loc["name_len"]], loc["index"], table)
            out[i] = (at + loc["text_off"], at + loc["name_off"], loc["text_len"], loc["name_len"], loc["index"],
                      UNBOUND if chunk is None else SEND_CHUNK)
        chunks.append(chunk)
    return out, chunks


def dense_expected(frames, chunks, table, max_chunks):
    """The six dense tables and n_located after a call, neutral entries included."""
    text_off = np.zeros(max_chunks, np.uint64)
    text_len = np.zeros(max_chunks, np.uint32)
    size = np.zeros(max_chunks, np.uint32)
    exp = np.zeros((max_chunks, 20), np.uint8)
    chunk_of = np.full(max_chunks, NONE, np.uint32)
    frame_of = np.full(max_chunks, NONE, np.uint32)
    j = 0
    for i, c in enumerate(chunks):
        if c is None:
            continue
        if j < max_chunks:
            text_off[j], text_len[j] = frames[i]["text_offset"], frames[i]["text_len"]
            size[j] = table[3][c]
            exp[j] = np.frombuffer(table[4][c], np.uint8)
            chunk_of[j], frame_of[j] = c, i
        j += 1
    return text_off, text_len, size, exp.reshape(-1), chunk_of, frame_of, j


# ---- frame builders --------------------------------------------------------
def _frame(body: bytes) -> bytes:
    return body.replace(b"\n", b" ").replace(b"\r", b" ") + b"\n"


def base64_put(data: bytes) -> bytes:
    """PeerWire::Base64Put: a newline behind every 18th whole group, no newline behind a padded group."""
    text = base64.b64encode(data)
    whole = len(data) // 3
    out = bytearray()
    for g in range(0, len(text), 4):
        out += text[g:g + 4]
        if g // 4 < whole and g // 4 % 18 == 17:
            out += b"\n"
    return bytes(out)


def send_chunk_text(name: bytes, index: int, text: bytes, idx: bytes = None, escape=xml_encode) -> bytes:
    """PeerWire::FrameSendChunkText: the frame around a chunk's text in either layout; idx overrides the digits."""
    if idx is None:
        idx = b"%d" % (index - (1 << 32) if index >= 1 << 31 else index)
    head = (REQUEST_BEGIN + b"SendChunk" + REQUEST_END_NAME + b"<params><param><value>" + escape(name) +
            b"</value></param><param><value><i4>" + idx + b"</i4></value></param><param><value><base64>")
    tail = b"</base64></value></param></params>" + REQUEST_END
    return _frame(head)[:-1] + text + _frame(tail)


def encode_send_chunk(name: bytes, index: int, data: bytes) -> bytes:
    """PeerWire::EncodeSendChunk (the xmlrpc++ layout, newlines as spaces)."""
    return send_chunk_text(name, index, base64_put(data).replace(b"\n", b" "))


def encode_send_chunk_flat(name: bytes, index: int, data: bytes) -> bytes:
    """The frame a Java or Perl peer sends: unbroken base64."""
    return send_chunk_text(name, index, base64.b64encode(data))


def encode_method(method: bytes, params) -> bytes:
    """PeerWire::EncodeMethod; a param is bytes (a string), an int (an i4) or a bytearray (base64)."""
    body = REQUEST_BEGIN + method + REQUEST_END_NAME
    if params:
        body += b"<params>"
        for v in params:
            if isinstance(v, bytearray):
                body += b"<param><value><base64>" + base64_put(bytes(v)) + b"</base64></value></param>"
            elif isinstance(v, int):
                body += b"<param><value><i4>%d</i4></value></param>" % v
            else:
                body += b"<param><value>" + xml_encode(v) + b"</value></param>"
        body += b"</params>"
    return _frame(body + REQUEST_END)


def sha1(data: bytes) -> bytes:
    return hashlib.sha1(data).digest()


# ---- the corpus ------------------------------------------------------------
def hand_built_frames(search_trip: int):
    """The frames the issue lists for the locate kernel, without their delimiters: [(label, frame)]."""
    nm, d = b"dir/file.bin", bytes(range(7))
    base = encode_send_chunk(nm, 3, d)[:-1]
    out = []
    for size in (0, 1, 2, 3, 54, 55, (2 * search_trip + 1) * 3 // 4 + 3):
        out.append(("size %d" % size, encode_send_chunk(nm, 1, bytes((7 * k + size) & 255 for k in range(size)))[:-1]))
    for label, name in (("lt", b"a<b"), ("gt", b"a>b"), ("amp", b"a&b"), ("apos", b"a'b"), ("quot", b'a"b'),
                        ("empty name", b""), ("leading space", b"  \tx y")):
        out.append(("name " + label, encode_send_chunk(name, 2, d)[:-1]))
    out.append(("string tag", base.replace(b"<value>" + nm, b"<value><string>" + nm + b"</string>")))
    out.append(("string tag spaced", base.replace(b"<value>" + nm, b"<value> \t<string>" + nm + b"</string>")))
    out.append(("blank string", base.replace(b"<value>" + nm + b"</value>", b"<value>  </value>")))
    out.append(("int tag", base.replace(b"<i4>3</i4>", b"<int>3</int>")))
    out.append(("int tag, i4 end", base.replace(b"<i4>3</i4>", b"<int>3</i4>")))
    out.append(("spaced", re.sub(rb">(?=<)", b"> \t \r", base)))
    out.append(("no /param", base.replace(b"</param>", b"")))
    out.append(("no /value", base.replace(b"</value>", b"")))
    for idx in (b"0", b"-1", b"+7", b" 12", b"2147483647", b"2147483648", b"4294967296", b"-2147483649",
                b"9" * 20, b"-" + b"9" * 20, b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808",
                b"-9223372036854775809", b"1" * 62, b"-" + b"1" * 62, b"1" * 63, b"7" * 70, b"", b"+", b"-", b"x1",
                b"12x", b"1 ", b"\v\f12", b"+-3", b"0x10", b"00012"):
        out.append(("index %r" % idx, send_chunk_text(nm, 0, b"QUJD", idx=idx)[:-1]))
    out.append(("missing /i4", base.replace(b"</i4>", b"")))
    out.append(("RequestChunk", encode_method(b"RequestChunk", [nm, 5])[:-1]))
    out.append(("NotifyHaveChunk", encode_method(b"NotifyHaveChunk", [nm, 5])[:-1]))
    out.append(("SendChunk by EncodeMethod", encode_method(b"SendChunk", [nm, 5, bytearray(d)])[:-1]))
    out.append(("empty", b""))
    out.append(("unfinished methodName first", b"<methodName " + base))
    out.append(("SendChunkX", base.replace(b"SendChunk<", b"SendChunkX<")))
    out.append(("XSendChunk", base.replace(b">SendChunk", b">XSendChunk")))
    out.append(("second params", base.replace(b"</params>", b"</params><params>")))
    out.append(("doubled params", base.replace(b"<params>", b"<params><params>")))
    out.append(("params before methodName", b"<params>" + base))
    out.append(("name is i4", base.replace(b"<value>" + nm + b"</value>", b"<value><i4>1</i4></value>")))
    out.append(("index is string", base.replace(b"<i4>3</i4>", b"three")))
    out.append(("text is string", base.replace(b"<base64>", b"<string>")))
    out.append(("unknown tag", base.replace(b"<value>" + nm, b"<value><nil/>" + nm)))
    cut = base[:base.index(b"</base64>")]
    out.append(("no < behind the text", cut))
    out.append(("< is the last byte", cut + b"<"))
    out.append(("ends in <base64>", base[:base.index(b"<base64>") + 8]))
    out.append(("ends in <value>", base[:base.index(b"<value>") + 7]))
    out.append(("white space only", b" \t\r\v\f  "))
    return out


def mutated_frames(rng, count: int):
    """SendChunk frames with a few bytes changed, dropped or doubled; rates chosen so that between a tenth and nine
    tenths of them still locate (tests/test_wire_frames_cpu.py asserts it)."""
    pool = b"<>/ \t&;ivpx0-+9"
    out = []
    for k in range(count):
        data = rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        f = bytearray(encode_send_chunk(b"f%d&<.bin" % k, int(rng.integers(0, 1000)), data)[:-1])
        for _ in range(int(rng.integers(0, 4))):
            at = int(rng.integers(0, len(f)))
            what = int(rng.integers(0, 3))
            if what == 0:
                f[at] = pool[int(rng.integers(0, len(pool)))]
            elif what == 1:
                del f[at]
            else:
                f.insert(at, f[at])
        out.append(bytes(f))
    return out
