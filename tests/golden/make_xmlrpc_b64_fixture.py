"""Record tests/golden/xmlrpc07_base64_get.json (run where the reference
exists: `make -C oracle ref` builds oracle/xmlrpc_b64_driver.cpp against
xmlrpc++ 0.7's base64.h).

The junk, '=' and truncation rules of xmlrpc++'s decoder (base64.h:215-330)
were pinned by code reading alone: tests/wire_layouts.py b64get and
PeerWire::Base64Get are two restatements that agree with each other.  This
keeps what the reference's own decoder and encoder answer, as data:

  get: texts of chunks of 0..6 bytes with every damage kind of
       wire_layouts.damage at every position, and the text of a 55-byte chunk
       (a line, its separator and a padded group) with every kind at the ten
       positions around the separator; per text the decoded bytes, the
       iostatus and how many characters the decoder consumed.
  put: chunks of 0..8, 53..57 and 107..109 bytes and the encoder's text (its
       line breaks are '\\n'; the frame sends them as spaces).

Inputs and recorded outputs only.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import wire_layouts as W  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "xmlrpc_b64_driver")
OUT = os.path.join(HERE, "xmlrpc07_base64_get.json")


def fixture_chunk(n: int) -> bytes:
    return bytes((37 * k + 11 * n + 5) & 255 for k in range(n))


def get_texts():
    texts = []
    for n in range(7):
        t = W.xmlrpc_text(fixture_chunk(n))
        texts.append(t)
        for kind in W.KINDS:
            texts += [W.damage(t, kind, p) for p in W.positions(len(t), kind)]
    t = W.xmlrpc_text(fixture_chunk(55))
    assert len(t) == 77 and t[72:73] == b" "
    texts.append(t)
    for kind in W.KINDS:
        texts += [W.damage(t, kind, p) for p in range(67, 77)]
    return sorted(set(texts), key=lambda x: (len(x), x))


def put_chunks():
    return [fixture_chunk(n) for n in list(range(9)) + list(range(53, 58)) + [107, 108, 109]]


def drive(mode, items):
    lines = "".join((b.hex() or "-") + "\n" for b in items)
    out = subprocess.run([DRIVER, mode], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(items)
    return out


def main():
    if not os.path.exists(DRIVER):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
    texts, chunks = get_texts(), put_chunks()
    get = []
    for t, line in zip(texts, drive("get", texts)):
        o, status, used = line.split()
        get.append([t.hex(), "" if o == "-" else o, int(status), int(used)])
    put = [[d.hex(), "" if line == "-" else line] for d, line in zip(chunks, drive("put", chunks))]
    doc = {"source": "cpp/extern/xmlrpc++/0.7/src/base64.h:154-348 (base64<char>::put and ::get), called as "
                     "XmlRpcValue.cpp:417-455 calls them, through oracle/xmlrpc_b64_driver.cpp",
           "get_columns": ["text (hex)", "decoded bytes (hex)", "iostatus", "characters consumed"],
           "get": get,
           "put_columns": ["chunk (hex)", "text (hex)"],
           "put": put}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(get)} get and {len(put)} put records -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
