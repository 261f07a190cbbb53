"""lbf_wire_frames_launch and lbf_wire_send_chunks_launch, the parts that need
no GPU: tests/wire_frame_model.py pinned against the C++ it restates
(PeerWire::LocateSendChunk, EncodeSendChunk, XmlEncode through
tests/c/locate_lines.cpp), the four symbols and their bindings, the work
formulas, every refusal the launches make before they enqueue anything, the
kernel set of wire_frames.hip and its kernels' resource usage on gfx950,
wire_flood_table / xml_encode against the model and Flood::WireTable against
wire_flood_table (tests/c/wire_table_lines.cpp, also under ASan + UBSan as a
plain executable)."""
import inspect
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from bitflood_amd import _capi
from tests import wire_frame_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
HOST = os.path.join(ROOT, "bitflood_amd", "host")
LIBDIR = os.path.dirname(_capi.LIB_PATH)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNIT = "wire_frames.hip"
KERNELS = ("wire_split_count_kernel", "wire_scan_kernel", "wire_split_scatter_kernel", "wire_split_finish_kernel",
           "wire_locate_kernel", "wire_bind_kernel", "wire_bind_count_kernel", "wire_bind_scatter_kernel",
           "wire_neutral_kernel")
SYMBOLS = ("lbf_wire_frames_launch", "lbf_wire_frames_launch_work", "lbf_wire_send_chunks_launch",
           "lbf_wire_send_chunks_launch_work")
FRAMES, CHUNKS = b"lbf_wire_frames_launch", b"lbf_wire_send_chunks_launch"
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def build_program(tmp, source, name, extra=(), sources=()):
    """tests/c/<source> against libbitflood.so (or, with `sources`, against those host sources compiled with it)."""
    exe = str(tmp / name)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra,
                         "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", source), *sources,
                         "-o", exe, "-L" + LIBDIR, *([] if sources else ["-lbitflood"]), "-llbfhash",
                         "-Wl,-rpath," + LIBDIR, "-lpthread"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def locate_lines(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("locate_lines"), "locate_lines.cpp", "locate_lines")


def _records(items):
    return b"".join(struct.pack("<I", len(b)) + b for b in items)


def cxx_locate(exe, frames):
    r = subprocess.run([exe, "locate"], input=_records(frames), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for line in r.stdout.decode().splitlines():
        w = line.split()
        out.append(None if w[0] == "0" else (int(w[1]), int(w[2]), int(w[3]),
                                             b"" if w[4] == "-" else bytes.fromhex(w[4])))
    assert len(out) == len(frames)
    return out


def model_locate(frame):
    loc = M.locate(frame)
    if loc is None:
        return None
    raw = frame[loc["name_off"]:loc["name_off"] + loc["name_len"]]
    return loc["index"], loc["text_off"], loc["text_len"], M.xml_decode(raw)


# ---- the model against the C++ ---------------------------------------------
def test_locate_model_is_the_host_function_on_the_hand_built_frames(locate_lines):
    from bitflood_amd import hashing
    cases = M.hand_built_frames(hashing.WIRE_SEARCH_TRIP)
    got = cxx_locate(locate_lines, [f for _, f in cases])
    for (label, frame), g in zip(cases, got):
        assert model_locate(frame) == g, label
    located = {label for (label, _), g in zip(cases, got) if g is not None}
    # the cases mean what their labels say
    for label in ("size 0", "size 55", "name amp", "name empty name", "string tag", "string tag spaced", "blank string",
                  "int tag", "spaced", "no /param", "no /value", "index b'-1'", "index b' 12'", "index b'" + "9" * 20 +
                  "'", "index b'" + "1" * 63 + "'", "SendChunk by EncodeMethod", "unfinished methodName first",
                  "second params", "< is the last byte"):
        assert label in located, label
    for label in ("int tag, i4 end", "index b'" + "7" * 70 + "'", "index b''", "index b'+'", "index b'12x'",
                  "missing /i4", "doubled params", "RequestChunk", "NotifyHaveChunk", "empty", "SendChunkX",
                  "XSendChunk", "name is i4", "index is string", "text is string", "unknown tag",
                  "no < behind the text", "ends in <base64>"):
        assert label not in located, label
    want = {b"-1": 0xFFFFFFFF, b"2147483648": 0x80000000, b"4294967296": 0, b"9" * 20: 0xFFFFFFFF,
            b"-" + b"9" * 20: 0, b"-2147483649": 0x7FFFFFFF, b"+7": 7, b"00012": 12, b"0x10": None}
    for (label, frame), g in zip(cases, got):
        for idx, value in want.items():
            if label == "index %r" % idx:
                assert (g[0] if g else None) == value, label


def test_locate_model_is_the_host_function_on_every_prefix(locate_lines):
    frame = M.encode_send_chunk(b"a&b", 12, b"\x01\x02\x03\x04")[:-1]
    prefixes = [frame[:k] for k in range(len(frame) + 1)]
    got = cxx_locate(locate_lines, prefixes)
    assert [model_locate(p) for p in prefixes] == got
    first = frame.index(b"</base64>") + 1
    assert [g is not None for g in got] == [k >= first for k in range(len(frame) + 1)]


def test_locate_model_is_the_host_function_on_mutated_frames(locate_lines):
    frames = M.mutated_frames(np.random.default_rng(20260101), 3000)
    got = cxx_locate(locate_lines, frames)
    bad = [f for f, g in zip(frames, got) if model_locate(f) != g]
    assert not bad, (len(bad), bad[0])
    located = sum(g is not None for g in got)
    print("located", located, "of", len(frames))
    assert located >= len(frames) // 10 and len(frames) - located >= len(frames) // 10


def test_builders_are_the_host_encoders(locate_lines):
    rng = np.random.default_rng(7)
    cases = [(b"dir/a b.bin", 0, b""), (b"<&>'\"", 5, b"x"), (b"", 4000000000, bytes(range(54))),
             (b"n", 2147483647, bytes(range(55))), (b"long", 7, rng.integers(0, 256, 1000, dtype=np.uint8).tobytes())]
    recs = []
    for name, index, data in cases:
        recs += [name, b"%d" % index, data]
    r = subprocess.run([locate_lines, "encode"], input=_records(recs), capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().split()
    assert [bytes.fromhex(x) for x in lines] == [M.encode_send_chunk(*c) for c in cases]
    assert M.encode_method(b"SendChunk", [b"n", 3, bytearray(b"abc")]) == M.encode_send_chunk(b"n", 3, b"abc")


def test_split_model():
    assert M.split(b"") == ([], 0)
    assert M.split(b"x") == ([], 0)
    assert M.split(b"\n") == ([(0, 0)], 1)
    assert M.split(b"ab\n\ncd\ne") == ([(0, 2), (3, 0), (4, 2)], 7)


# ---- the ABI ---------------------------------------------------------------
def test_the_four_symbols_are_declared_once_exported_and_bound(lib):
    text = open(_capi.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert name in _capi._SIGS and name in _capi.header_symbols()
        assert getattr(lib, name).argtypes == _capi._SIGS[name][1]
        assert len(re.findall(r"\b%s\s*\(" % name, code)) == 1, name
    assert len(_capi._SIGS["lbf_wire_frames_launch"][1]) == 9
    assert len(_capi._SIGS["lbf_wire_send_chunks_launch"][1]) == 24
    assert lib.lbf_abi_version() == 1
    for name, value in (("LBF_FRAME_OTHER", 0), ("LBF_FRAME_SEND_CHUNK", 1), ("LBF_FRAME_SEND_CHUNK_UNBOUND", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), text)


def test_python_helpers():
    import bitflood_amd
    from bitflood_amd import hashing
    for name in ("wire_frames_launch", "wire_frames_launch_work", "wire_send_chunks_launch",
                 "wire_send_chunks_launch_work", "WIRE_FRAME_DTYPE", "xml_encode", "wire_flood_table"):
        assert name in hashing.__all__ and getattr(bitflood_amd, name) is getattr(hashing, name)
    p = inspect.signature(hashing.wire_frames_launch).parameters
    assert list(p) == ["stream_buf", "stream_len", "frame_offsets", "frame_lens", "max_frames", "n_frames", "tail",
                       "work", "stream"]
    p = inspect.signature(hashing.wire_send_chunks_launch).parameters
    assert list(p)[:7] == ["stream_buf", "stream_len", "frame_offsets", "frame_lens", "n_frames", "frames", "work"]
    assert all(v.default in (None, 0) for k, v in list(p.items())[7:])
    d = hashing.WIRE_FRAME_DTYPE
    assert d.itemsize == 32 and d.names == ("text_offset", "name_offset", "text_len", "name_len", "index", "kind")
    assert [d.fields[n][1] for n in d.names] == [0, 8, 16, 20, 24, 28]
    assert (hashing.LBF_FRAME_OTHER, hashing.LBF_FRAME_SEND_CHUNK, hashing.LBF_FRAME_SEND_CHUNK_UNBOUND) == \
        (M.OTHER, M.SEND_CHUNK, M.UNBOUND)


def test_python_mirrors_the_kernels_geometry():
    from bitflood_amd import hashing
    hpp = open(os.path.join(CSRC, "wire_frames.hpp")).read()
    assert "constexpr uint32_t kSplitBlock = %d;" % hashing.WIRE_SPLIT_BLOCK in hpp
    assert "constexpr uint32_t kSearchTrip = %d;" % hashing.WIRE_SEARCH_TRIP in hpp
    assert "constexpr uint32_t kBindBlock = %d;" % hashing.WIRE_BIND_BLOCK in hpp
    assert "constexpr uint32_t kScanWidth = %d;" % hashing.WIRE_SCAN_WIDTH in hpp
    assert "constexpr uint64_t kMaxFrame = (3ull << 29) + (64ull << 10);" in hpp and M.MAX_FRAME == (3 << 29) + 65536
    assert hpp.count("constexpr uint32_t kSplitBlock") == 1 and "kSplitBlock =" not in open(
        os.path.join(CSRC, UNIT)).read()


@pytest.mark.parametrize("n", [0, 1, 4081, 4082, 4096, 8177, 8178, (1 << 32) - 1])
def test_split_work_is_the_documented_formula(lib, n):
    """include/lbf_hash.h: 4 * ceil((stream_len + 15) / 4096)."""
    from bitflood_amd import wire_frames_launch_work
    want = 4 * ((n + 15 + 4095) // 4096)
    assert lib.lbf_wire_frames_launch_work(n) == want == wire_frames_launch_work(n)
    assert "4 * ceil((stream_len + 15) / 4096)" in open(_capi.HEADER_PATH).read()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, (1 << 31) - 1])
def test_send_chunks_work_is_the_documented_formula(lib, n):
    """include/lbf_hash.h: 4 * n_frames + 4 * ceil(n_frames / 256)."""
    from bitflood_amd import wire_send_chunks_launch_work
    want = 4 * n + 4 * ((n + 255) // 256)
    assert lib.lbf_wire_send_chunks_launch_work(n) == want == wire_send_chunks_launch_work(n)
    assert "4 * n_frames + 4 * ceil(n_frames / 256)" in open(_capi.HEADER_PATH).read()


# ---- the refusals ----------------------------------------------------------
def _refused(lib, rc, who, *words):
    msg = lib.lbf_last_error() or b""
    assert rc == _capi.LBF_ERR_INVALID, (rc, msg)
    assert msg.startswith(who + b":"), msg
    for w in words:
        assert w in msg, (w, msg)


def _tables(n=2):
    """Host arrays standing in for every table of the two calls (the refusals come before any of them is read)."""
    return dict(stream=np.zeros(64, np.uint8), foff=np.zeros(n + 1, np.uint64), flen=np.zeros(n + 1, np.uint32),
                nfr=np.zeros(2, np.uint32), tail=np.zeros(2, np.uint64), work=np.zeros(64, np.uint32),
                names=np.zeros(8, np.uint8), noff=np.zeros(3, np.uint32), first=np.zeros(3, np.uint32),
                sizes=np.zeros(3, np.uint32), exp=np.zeros(64, np.uint8), frames=np.zeros(n + 1, [("a", "<u8", 4)]),
                toff=np.zeros(3, np.uint64), tlen=np.zeros(3, np.uint32), esz=np.zeros(3, np.uint32),
                dexp=np.zeros(64, np.uint8), cof=np.zeros(3, np.uint32), fof=np.zeros(3, np.uint32),
                nloc=np.zeros(2, np.uint32))


def _ptrs(t, null, shift):
    return {k: (None if k in null else v.ctypes.data + (shift or {}).get(k, 0)) for k, v in t.items()}


def _frames(lib, t, stream_len=16, max_frames=2, null=(), shift=None):
    p = _ptrs(t, null, shift)
    return lib.lbf_wire_frames_launch(p["stream"], stream_len, p["foff"], p["flen"], max_frames, p["nfr"], p["tail"],
                                      p["work"], None)


TABLE = ("names", "noff", "first", "sizes", "exp")
DENSE = ("toff", "tlen", "esz", "dexp", "cof", "fof", "nloc")


def _chunks(lib, t, n_frames=2, null=(), shift=None, n_files=1, n_chunks=2, max_chunks=2, stream_len=16):
    p = _ptrs(t, null, shift)
    return lib.lbf_wire_send_chunks_launch(p["stream"], stream_len, p["foff"], p["flen"], n_frames, p["nfr"],
                                           p["names"], p["noff"], p["first"], n_files, p["sizes"], p["exp"], n_chunks,
                                           p["frames"], p["toff"], p["tlen"], p["esz"], p["dexp"], p["cof"], p["fof"],
                                           max_chunks, p["nloc"], p["work"], None)


@pytest.mark.parametrize("table", ["stream", "nfr", "tail", "work"])
def test_frames_launch_refuses_a_null_required_argument(lib, table):
    _refused(lib, _frames(lib, _tables(), null=(table,)), FRAMES, b"null")


def test_frames_launch_refuses_a_stream_past_32_bits(lib):
    _refused(lib, _frames(lib, _tables(), stream_len=1 << 32), FRAMES, b"2^32-1")


def test_frames_launch_refuses_half_of_the_frame_tables(lib):
    for null, mf in ((("foff",), 2), (("flen",), 2), (("foff", "flen"), 2), ((), 0)):
        _refused(lib, _frames(lib, _tables(), null=null, max_frames=mf), FRAMES, b"go together")


@pytest.mark.parametrize("table,by", [("foff", 4), ("flen", 2), ("nfr", 2), ("tail", 4), ("work", 2)])
def test_frames_launch_refuses_a_misaligned_table(lib, table, by):
    _refused(lib, _frames(lib, _tables(), shift={table: by}), FRAMES, b"not aligned to its element size")


@pytest.mark.parametrize("table", ["stream", "foff", "flen", "frames", "work"])
def test_send_chunks_launch_refuses_a_null_required_argument(lib, table):
    _refused(lib, _chunks(lib, _tables(), null=(table,)), CHUNKS, b"null")


@pytest.mark.parametrize("table", TABLE)
def test_send_chunks_launch_refuses_half_a_flood_table(lib, table):
    _refused(lib, _chunks(lib, _tables(), null=(table,)), CHUNKS, b"flood table", b"go together")
    rest = tuple(k for k in TABLE if k != table)
    _refused(lib, _chunks(lib, _tables(), null=rest, n_files=0, n_chunks=0), CHUNKS, b"flood table", b"go together")


def test_send_chunks_launch_refuses_counts_without_their_tables(lib):
    _refused(lib, _chunks(lib, _tables(), null=TABLE, n_files=1, n_chunks=2), CHUNKS, b"flood table")
    _refused(lib, _chunks(lib, _tables(), null=TABLE, n_files=0, n_chunks=2), CHUNKS, b"flood table")
    _refused(lib, _chunks(lib, _tables(), n_files=1, n_chunks=0), CHUNKS, b"n_files without n_chunks")
    _refused(lib, _chunks(lib, _tables(), null=DENSE, max_chunks=2), CHUNKS, b"dense tables")
    _refused(lib, _chunks(lib, _tables(), max_chunks=0), CHUNKS, b"dense tables")


@pytest.mark.parametrize("table", DENSE)
def test_send_chunks_launch_refuses_half_the_dense_tables(lib, table):
    _refused(lib, _chunks(lib, _tables(), null=(table,)), CHUNKS, b"dense tables", b"go together")
    rest = tuple(k for k in DENSE if k != table)
    _refused(lib, _chunks(lib, _tables(), null=rest, max_chunks=0), CHUNKS, b"dense tables", b"go together")


def test_send_chunks_launch_refuses_too_many(lib):
    _refused(lib, _chunks(lib, _tables(), n_frames=1 << 31), CHUNKS, b"n_frames exceeds 2^31-1")
    _refused(lib, _chunks(lib, _tables(), max_chunks=1 << 31), CHUNKS, b"max_chunks exceeds 2^31-1")


@pytest.mark.parametrize("table,by", [("foff", 4), ("flen", 2), ("nfr", 2), ("noff", 2), ("first", 2), ("sizes", 2),
                                      ("frames", 4), ("toff", 4), ("tlen", 2), ("esz", 2), ("cof", 2), ("fof", 2),
                                      ("nloc", 2), ("work", 2)])
def test_send_chunks_launch_refuses_a_misaligned_table(lib, table, by):
    _refused(lib, _chunks(lib, _tables(), shift={table: by}), CHUNKS, b"not aligned to its element size")


def test_tables_are_checked_against_their_allocations():
    """check_fits needs a device allocation to refuse anything (tests/test_gpu_wire_frames.py runs it); here, that
    every table of both calls is on the validator's list with its element size."""
    text = open(os.path.join(CSRC, UNIT)).read()
    assert text.count("lbf::tables_fit(who, tables)") == 2 and text.count("lbf::tables_aligned(who, tables)") == 2
    for row in ('{d_stream, 1, stream_len, "stream", false}', '{d_frame_offsets, 8, kept, "frame_offsets", true}',
                '{d_frame_lens, 4, kept, "frame_lens", true}', '{d_n_frames, 4, 1, "n_frames", true}',
                '{d_tail, 8, 1, "tail", true}', '{d_work, 4, wf::split_blocks(stream_len), "work", true}',
                '{nf ? d_stream : nullptr, 1, stream_len, "stream", false}',
                '{d_frame_offsets, 8, nf, "frame_offsets", true}', '{d_frame_lens, 4, nf, "frame_lens", true}',
                '{d_file_name_offsets, 4, (uint64_t)n_files + 1, "file_name_offsets", true}',
                '{d_file_first, 4, (uint64_t)n_files + 1, "file_first", true}',
                '{d_chunk_sizes, 4, n_chunks, "chunk_sizes", true}',
                '{d_chunk_expected, 20, n_chunks, "chunk_expected", false}', '{d_frames, 8, 4 * nf, "frames", true}',
                '{d_text_offsets, 8, max_chunks, "text_offsets", true}',
                '{d_text_lens, 4, max_chunks, "text_lens", true}',
                '{d_expected_sizes, 4, max_chunks, "expected_sizes", true}',
                '{d_expected, 20, max_chunks, "expected", false}', '{d_chunk_of, 4, max_chunks, "chunk_of", true}',
                '{d_frame_of, 4, max_chunks, "frame_of", true}', '{d_n_located, 4, 1, "n_located", true}',
                '{nf ? d_work : nullptr, 4, wf::bind_work_bytes(nf) / 4, "work", true}'):
        assert row in text, row


def test_nothing_to_do_is_ok(lib):
    t = _tables()
    t["nfr"][:] = 0xABCD
    t["tail"][:] = 0xABCD
    assert lib.lbf_wire_frames_launch(None, 0, None, None, 0, None, None, None, None) == 0
    assert _frames(lib, t, stream_len=0) == 0
    assert (t["nfr"] == 0xABCD).all() and (t["tail"] == 0xABCD).all()  # nothing is written
    # no frames and no dense tables: nothing to enqueue, whatever else is NULL
    assert lib.lbf_wire_send_chunks_launch(None, 0, None, None, 0, None, None, None, None, 0, None, None, 0, None,
                                           None, None, None, None, None, None, 0, None, None, None) == 0
    assert _chunks(lib, t, n_frames=0, null=DENSE + ("stream", "foff", "flen", "frames", "work"), max_chunks=0) == 0
    # the group checks come first
    _refused(lib, _chunks(lib, t, n_frames=0, null=("toff",)), CHUNKS, b"dense tables")


# ---- the unit --------------------------------------------------------------
@needs_hipcc
def test_the_new_source_holds_exactly_its_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_digest
    got = isa_digest.digests(os.path.join(CSRC, UNIT))
    assert len(got) == len(KERNELS), sorted(got)
    for k in KERNELS:
        assert sum(k + "E" in name for name in got) == 1, (k, sorted(got))
    srcs = subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True, text=True,
                          check=True).stdout.split()
    assert UNIT in srcs


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("wire_frames") / "k.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--offload-device-only", "-c", "-o", str(out),
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, UNIT)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return re.split(r"remark: Function Name: ", r.stderr)[1:]


@needs_hipcc
@pytest.mark.parametrize("kernel", KERNELS)
def test_kernels_have_no_scratch_no_spills_and_no_dynamic_stack(remarks, kernel):
    found = [b for b in remarks if kernel + "E" in b.split()[0]]
    assert len(found) == 1, [b.split()[0] for b in remarks]
    rem = found[0]
    print(rem)
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem), rem
    assert re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem
    assert re.search(r"Dynamic Stack: False", rem), rem


def test_scan_comes_from_the_shared_header_and_nothing_is_atomic():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert '#include "b64_device.hpp"' in text
    code = re.sub(r"//[^\n]*", "", text)
    assert code.count("b64d::wg_exclusive_scan<") >= 4
    assert "atomic" not in code.lower() and "__shfl_up" not in code
    assert len(re.findall(r"__global__", code)) == len(KERNELS)


# ---- the flood table -------------------------------------------------------
def _floods():
    rng = np.random.default_rng(3)
    dig = lambda n: [rng.integers(0, 256, 20, dtype=np.uint8).tobytes() for _ in range(n)]  # noqa: E731
    return [[], [(b"one", [5], dig(1))],
            [(b"a", [262144, 262144, 17], dig(3)), (b"a<b>&'\".bin", [], []), (b"ab", [1, 2], dig(2)),
             (b"", [9], dig(1)), (b"z/\xc3\xa9 y", [0], dig(1))]]


def test_xml_encode_is_the_model_and_undone_by_xml_decode():
    from bitflood_amd import xml_encode
    for raw in (b"", b"plain", b"<>&'\"", b"a&amp;b", b"&lt", bytes(range(1, 256))):
        assert xml_encode(raw) == M.xml_encode(raw)
        assert M.xml_decode(xml_encode(raw)) == raw
    assert xml_encode("a<b") == b"a&lt;b" and xml_encode(b"&") == b"&amp;" and xml_encode(b"'\"") == b"&apos;&quot;"


@pytest.mark.parametrize("which", [0, 1, 2])
def test_wire_flood_table_is_the_model(which):
    from bitflood_amd import wire_flood_table
    files = _floods()[which]
    names, noff, first, sizes, exp = wire_flood_table(files)
    m = M.flood_table(files)
    assert names.dtype == np.uint8 and names.tobytes() == b"".join(m[0])
    assert noff.dtype == np.uint32 and noff.tolist() == m[1]
    assert first.dtype == np.uint32 and first.tolist() == m[2]
    assert sizes.dtype == np.uint32 and sizes.tolist() == m[3]
    assert exp.dtype == np.uint8 and exp.tobytes() == b"".join(m[4])
    for f, (name, fs, _) in enumerate(files):
        for k in range(len(fs)):
            assert M.bind(M.xml_encode(name), k, m) == first[f] + k
        assert M.bind(M.xml_encode(name), len(fs), m) is None
    assert M.bind(b"nowhere", 0, m) is None


def test_wire_flood_table_refuses_a_short_digest():
    from bitflood_amd import wire_flood_table
    with pytest.raises(ValueError):
        wire_flood_table([(b"a", [1], [b"short"])])
    with pytest.raises(ValueError):
        wire_flood_table([(b"a", [1, 2], [bytes(20)])])


@pytest.mark.parametrize("name,extra,own", [("plain", [], False),
                                            ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
                                             True)])
def test_flood_wire_table_is_wire_flood_table(tmp_path, name, extra, own):
    """Flood::WireTable from a flood whose files and chunks arrive out of order, against wire_flood_table; the second
    build compiles the host sources with the sanitizers into the program itself (a plain executable)."""
    from bitflood_amd import b64_27, wire_flood_table
    sources = [os.path.join(HOST, s) for s in ("Flood.cpp", "FloodFile.cpp", "Encoder.cpp", "PeerWire.cpp",
                                               "PieceHasher.cpp")] if own else []
    exe = build_program(tmp_path, "wire_table_lines.cpp", "wire_table_lines_" + name, extra, sources)
    files = _floods()[2]
    lines = []
    for fname, fs, fd in reversed(files):  # the map sorts the names
        lines.append("F " + (fname.hex() or "-"))
        for k in reversed(range(len(fs))):
            lines.append("C %d %d %s" % (k, fs[k], b64_27(fd[k])))
    lines.append("F " + b"bad".hex())
    lines.append("C 0 3 not-a-canonical-hash-string")
    files = sorted(files + [(b"bad", [3], [bytes(20)])])
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                       env={**os.environ, "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert out[0] == "ok", r.stdout
    names, noff, first, sizes, exp = wire_flood_table(files)
    assert (b"" if out[1] == "-" else bytes.fromhex(out[1])) == names.tobytes()
    assert [int(x) for x in out[2].split()] == noff.tolist()
    assert [int(x) for x in out[3].split()] == first.tolist()
    assert [int(x) for x in out[4].split()] == sizes.tolist()
    assert [int(x) for x in out[5].split()] == exp.tolist()
