"""The device-resident launch paths (lbf_sha1_uniform_launch, lbf_sha1_launch)
swept over block counts and start alignment, against the oracle.

These entry points are what bench.py times and the sharded ranks call; their
uniform form runs separately compiled kernels (kUniform = true).  The layouts
come from tests/device_layouts.py, and tests/test_device_layouts.py shows on
the CPU what they reach: every exit residue of the fast loops of pc4 (8 steps a
trip) and pc4x2 / pcx5 (6) after two or more full trips, short chains that end
inside and just behind the fast loop, chunks at every start residue mod 16,
every tail edge.  No chain is longer than 27 block steps.

The expected value is always oracle.sha1_batch on the same host bytes and every
comparison is equality.  Output arrays are pre-filled with 0xA5, so a result
that was never written cannot pass for one left over from an earlier launch.
"""
import numpy as np
import pytest

from bitflood_amd import DeviceBuffer, _capi
from bitflood_amd import hashing as H
from tests import device_layouts as L

pytestmark = pytest.mark.gpu

VARIANTS = [1, 7, 10, 11, 12]
FILL = 0xA5


@pytest.fixture(params=VARIANTS, ids=lambda v: {1: "lane", 7: "pc4b64", 10: "pcx5", 11: "lds2", 12: "pc4x2"}[v])
def variant(request):
    H.set_kernel_variant(request.param)
    yield request.param
    H.set_kernel_variant(0)


def _frozen(a):
    a.setflags(write=False)
    return a


def _with_ref(oracle, t):
    return t, _frozen(oracle.sha1_batch(t.data, t.offsets, t.sizes, nthreads=8))


@pytest.fixture(scope="module")
def level(oracle):
    """Every level_table ordering with its oracle digests, computed once."""
    return [_with_ref(oracle, t) for t in L.level_table(64) + L.level_table(128)]


@pytest.fixture(scope="module")
def ragged(oracle):
    return _with_ref(oracle, L.ragged_table())


@pytest.fixture(scope="module")
def uniform(oracle):
    """(case, oracle digests) of every uniform case, over one seeded stream."""
    cases = L.uniform_cases()
    stream = _frozen(np.random.default_rng(3000).integers(0, 256, max(c[2] for c in cases), dtype=np.uint8))
    refs = [_frozen(oracle.sha1_batch(stream, *L.uniform_table(cs, n, length))) for cs, n, length, _ in cases]
    return stream, cases, refs


class Device:
    """Device buffers of one test, freed together."""

    def __init__(self):
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()

    def alloc(self, nbytes):
        self.bufs.append(DeviceBuffer(max(int(nbytes), 1)))
        return self.bufs[-1]

    def put(self, host, offset=0):
        host = np.ascontiguousarray(host)
        b = self.alloc(offset + host.nbytes)
        if host.nbytes:
            b.upload(host, offset)
        return b

    def filled(self, nbytes):
        return self.put(np.full(max(int(nbytes), 1), FILL, dtype=np.uint8))


def _rows(buf, n):
    return buf.download(20 * n).reshape(n, 20)


def _assert_rows(got, want, describe, what):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} wrong, first: " + " | ".join(
        describe(i) for i in bad[:4])


def _uniform_describe(cs, n, length, shift, first=0):
    def describe(i):
        i = int(i) + first
        size = min(cs, length - i * cs)
        return (f"chunk {i} of uniform cs={cs} n={n} len={length} base_shift={shift}: T={L.steps(size)} "
                f"{L.tail_form(size & 63)} tail (r={size & 63}) start residue {(shift + i * cs) % 16} mod 16, "
                f"lane {(i - first) % 64} of wave {(i - first) // 64}")
    return describe


def _flip_expected(exp, flips):
    """One bit of byte 0, 7 or 19 of each listed digest."""
    for k, i in enumerate(flips):
        exp[i, (0, 7, 19)[k % 3]] ^= 1 << (k % 8)
    return exp


def _verdict_pattern(n, zeros):
    v = np.ones(n, dtype=np.uint8)
    v[list(zeros)] = 0
    return v


# ---------------------------------------------------------------------------
def test_level_tables_three_ways(variant, hasher, level):
    """Runs of 64 / 128 equal chains, T = 1..26 in both tail forms, aligned and
    not: the host-staged path, lbf_sha1_launch and lbf_sha1_batch with
    LBF_DEVICE_PTR all equal the oracle."""
    lib = _capi.load()
    for t, want in level:
        n = t.n
        _assert_rows(hasher.hash_chunks(t.data, t.offsets, t.sizes), want, t.describe, "hash_chunks")
        with Device() as dev:
            d_data, d_off, d_size = dev.put(t.data), dev.put(t.offsets), dev.put(t.sizes)
            d_out = dev.filled(20 * n)
            H.batch_launch(d_data, d_off, d_size, n, d_out)
            H.synchronize()
            _assert_rows(_rows(d_out, n), want, t.describe, "lbf_sha1_launch")
            d_out2 = dev.filled(20 * n)
            _capi.check(lib.lbf_sha1_batch(hasher._h, d_data.ptr, t.data.size, d_off.ptr, d_size.ptr, n, d_out2.ptr,
                                           _capi.LBF_DEVICE_PTR))
            _assert_rows(_rows(d_out2, n), want, t.describe, "lbf_sha1_batch(LBF_DEVICE_PTR)")


def test_ragged_tables(variant, hasher, ragged):
    """One short chain among 63 long ones, ending inside and 1, 2, 7 or more
    steps before the end of its workgroup: hash mode, and verify mode with the
    short chain's and one long chain's expected digest off by a bit."""
    t, want = ragged
    n = t.n
    flips = []
    for k, run in enumerate(t.runs):
        long_lane = (7 * k) % 64
        flips += [run.start + L.SHORT_LANE, run.start + (long_lane if long_lane != L.SHORT_LANE else 63)]
    exp = _flip_expected(want.copy(), flips)
    pattern = _verdict_pattern(n, flips)

    _assert_rows(hasher.hash_chunks(t.data, t.offsets, t.sizes), want, t.describe, "hash_chunks")
    v = hasher.verify_chunks(t.data, t.offsets, t.sizes, exp)
    _assert_rows(v.astype(np.uint8), pattern, t.describe, "verify_chunks verdicts")
    with Device() as dev:
        d_data, d_off, d_size = dev.put(t.data), dev.put(t.offsets), dev.put(t.sizes)
        d_out = dev.filled(20 * n)
        H.batch_launch(d_data, d_off, d_size, n, d_out)
        H.synchronize()
        _assert_rows(_rows(d_out, n), want, t.describe, "lbf_sha1_launch")
        d_exp, d_ver = dev.put(exp), dev.filled(n)
        H.batch_launch(d_data, d_off, d_size, n, None, expected=d_exp, verdicts=d_ver)
        H.synchronize()
        _assert_rows(d_ver.download(n), pattern, t.describe, "lbf_sha1_launch verdicts")


def test_uniform_odd_chunk_sizes(variant, uniform):
    """lbf_sha1_uniform_launch at odd chunk sizes (chunks at every start
    residue; the kUniform kernels' misaligned branches) and at multiples of
    16, from a base 0 and 3 bytes into a buffer that ends with the region.
    Every third case again as a sub-range (first_chunk > 0)."""
    stream, cases, refs = uniform
    fill = np.full(20 * 129, FILL, dtype=np.uint8)
    with Device() as dev:
        dig = dev.alloc(fill.size)
        for idx, ((cs, n, length, shift), want) in enumerate(zip(cases, refs)):
            buf = DeviceBuffer(shift + length)
            try:
                buf.upload(stream[:length], shift)
                dig.upload(fill)
                H.uniform_launch(buf.ptr + shift, length, cs, 0, n, dig)
                H.synchronize()
                _assert_rows(_rows(dig, n), want, _uniform_describe(cs, n, length, shift), "uniform launch")
                if idx % 3 == 0:
                    first = (1, 5, 63)[(idx // 3) % 3]
                    dig.upload(fill)
                    H.uniform_launch(buf.ptr + shift, length, cs, first, n - first, dig)
                    H.synchronize()
                    _assert_rows(_rows(dig, n - first), want[first:], _uniform_describe(cs, n, length, shift, first),
                                 f"uniform launch from chunk {first}")
            finally:
                buf.free()


def _idle_table(n):
    """n misaligned chains, the first of each wave the longest."""
    rng = np.random.default_rng(4000 + n)
    sizes = rng.integers(0, 900, n).astype(np.uint32)
    res = rng.integers(1, 16, n)
    for w0 in range(0, n, 64):
        sizes[w0] = L.size_for(20, L.TAIL_TWO) + w0  # 20 steps or more; the others have at most 15
        res[w0] = 5
    offs, pos = [], 0
    for s, r in zip(sizes.tolist(), res.tolist()):
        offs.append((pos + 15) // 16 * 16 + r)
        pos = offs[-1] + s
    data = rng.integers(0, 256, pos, dtype=np.uint8)
    return data, np.array(offs, dtype=np.uint64), sizes


@pytest.mark.parametrize("n", [1, 63, 65, 127, 129, 191])
def test_idle_lanes_write_nothing(variant, oracle, n):
    """Lanes past the end of the table run a copy of their wave's first chain
    (kern_common.hpp chain_info) and must store nothing: the digest and verdict
    arrays have room for 128 more entries, and every byte past the n-th entry
    still holds its fill after the launch."""
    room = n + 128
    describe = lambda i: f"entry {int(i)} of {n}"  # noqa: E731
    cs = L.size_for(7, L.TAIL_ONE)  # odd: chunks misaligned
    length = (n - 1) * cs + 100
    data, offs, sizes = _idle_table(n)
    u_data = np.random.default_rng(4500 + n).integers(0, 256, length, dtype=np.uint8)
    launches = []
    with Device() as dev:
        d_u = dev.put(u_data, offset=3)
        launches.append(("uniform", oracle.sha1_batch(u_data, *L.uniform_table(cs, n, length)),
                         lambda *out: H.uniform_launch(d_u.ptr + 3, length, cs, 0, n, *out)))
        d_data, d_off, d_size = dev.put(data), dev.put(offs), dev.put(sizes)
        launches.append(("table", oracle.sha1_batch(data, offs, sizes),
                         lambda *out: H.batch_launch(d_data, d_off, d_size, n, *out)))
        for name, want, launch in launches:
            exp = np.full((room, 20), FILL, dtype=np.uint8)
            exp[:n] = want
            d_dig, d_exp, d_ver = dev.filled(20 * room), dev.put(exp), dev.filled(room)
            launch(d_dig, d_exp, d_ver)
            H.synchronize()
            dig, ver = d_dig.download(20 * room), d_ver.download(room)
            _assert_rows(dig[:20 * n].reshape(n, 20), want, describe, f"{name} digests")
            _assert_rows(ver[:n], np.ones(n, np.uint8), describe, f"{name} verdicts")
            stray = np.flatnonzero(dig[20 * n:] != FILL)
            assert stray.size == 0, f"{name}: digest bytes written past entry {n}, at {20 * n + stray[:8]}"
            stray = np.flatnonzero(ver[n:] != FILL)
            assert stray.size == 0, f"{name}: verdict bytes written past entry {n}, at {n + stray[:8]}"


@pytest.mark.parametrize("form", ["uniform", "table"])
def test_device_verify_mismatches_and_both_outputs(variant, oracle, form):
    """A device launch with digests, expected and verdicts all set writes both
    outputs; verdicts are 0 exactly where the expected digest is off by one bit
    (byte 0, 7 or 19) or the chunk's last data byte is, first and last (short)
    chunk and lanes 63 and 64 among them.  Then the same with digests = None."""
    n = 200
    rng = np.random.default_rng(5000)
    if form == "uniform":
        cs = L.size_for(10, L.TAIL_ONE)
        length = (n - 1) * cs + 50
        offs, sizes = L.uniform_table(cs, n, length)
        describe = _uniform_describe(cs, n, length, 0)
    else:
        sizes = rng.integers(1, 1700, n).astype(np.uint32)
        sizes[-1] = 9
        offs = (np.concatenate([[0], np.cumsum(sizes[:-1] + 21, dtype=np.uint64)])).astype(np.uint64)
        length = int(offs[-1]) + int(sizes[-1])
        describe = lambda i: (f"entry {int(i)}: size {int(sizes[i])} T={L.steps(int(sizes[i]))} "  # noqa: E731
                              f"start residue {int(offs[i]) % 16} mod 16")
    pristine = rng.integers(0, 256, length, dtype=np.uint8)
    exp_flips = [0, 63, 64, 131]
    data_flips = [n - 1, 130, 17]
    data = pristine.copy()
    for k, i in enumerate(data_flips):
        data[int(offs[i]) + int(sizes[i]) - 1] ^= 1 << (2 * k + 1)
    want = oracle.sha1_batch(data, offs, sizes)
    exp = _flip_expected(oracle.sha1_batch(pristine, offs, sizes), exp_flips)
    pattern = _verdict_pattern(n, exp_flips + data_flips)
    with Device() as dev:
        d_data, d_exp = dev.put(data), dev.put(exp)
        if form == "uniform":
            launch = lambda *out: H.uniform_launch(d_data, length, cs, 0, n, *out)  # noqa: E731
        else:
            d_off, d_size = dev.put(offs), dev.put(sizes)
            launch = lambda *out: H.batch_launch(d_data, d_off, d_size, n, *out)  # noqa: E731
        d_dig, d_ver = dev.filled(20 * n), dev.filled(n)
        launch(d_dig, d_exp, d_ver)
        H.synchronize()
        _assert_rows(_rows(d_dig, n), want, describe, "digests")
        _assert_rows(d_ver.download(n), pattern, describe, "verdicts")
        d_ver2 = dev.filled(n)
        launch(None, d_exp, d_ver2)
        H.synchronize()
        _assert_rows(d_ver2.download(n), pattern, describe, "verdicts with digests = None")
