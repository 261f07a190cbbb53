"""The device-resident launch paths the way a receiver runs them: eight streams
in flight, a decode on one while a hash runs on another, round chained behind
round on a stream with the states left in HBM and no host wait between them
(lbf_b64_update_launch, lbf_sha1_update_launch, lbf_sha1_uniform_launch;
DESIGN.md §5.1, "two verifies in flight").

The other device-resident tests wait on their stream after every launch and
read back with a blocking copy, with nothing else in flight: a kernel sent to
the null stream, or to another stream than the caller's, would pass them.
Here every stream starts with a plug (one chain of 8 MiB, about 0.1 s), so all
that is enqueued behind it waits while a kernel on the wrong stream runs ahead
of its inputs; all tables are uploaded before the first enqueue and everything
is read back after the last.  The work, what it must leave behind and the check
are tests/stream_feed.py's; expected values come from the models, hashlib and
the oracle, never from a GPU path.
"""
import json
import os
import subprocess
import sys

import pytest

from bitflood_amd import hashing as H
from tests import stream_feed as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("variant", [0, 1, 10], ids=["auto", "lane", "pcx5"])
def test_chained_rounds_on_four_streams_without_a_host_wait(variant):
    """Four decode streams over one arena whose touching slots go round the
    streams (neighbours share 16-byte blocks), the six routes cycling launch by
    launch so that different routes are in flight together; behind each round a
    round of raw-byte updates on two more streams and a hash launch on one of
    two more, its shape cycling through the three kernels auto picks (or the
    forced lane / pcx5 kernel, which auto never picks).  Chains end in
    different rounds; cap + 1 and cap - 1 chains get their verdict 0 from
    b64_length_kernel alone; three chains per stream stay mid-chunk with 0..3
    sextets carried."""
    run = S.Run(S.one_thread_hash_keys())
    before = None
    try:
        H.set_kernel_variant(variant)
        before = S.set_route(S.ROUTES[0])
        S.enqueue_from_one_thread(run, route_of=lambda r, s: S.ROUTES[(4 * r + s) % 6])
        found = run.problems()
    finally:
        if before is not None:
            S.set_route(before)
        H.set_kernel_variant(0)
        run.close()
    assert run.plugged == set(range(S.STREAMS))
    assert not found, (len(found), found[:6])


def test_launches_from_four_threads_on_their_own_streams():
    """The same work enqueued by four host threads at once, each on a stream of
    its own: its plug, its decode rounds, a hash launch behind each, and for two
    of them a stream of raw-byte updates.  The switches stay at their defaults."""
    found = S.four_threads()
    assert not found, (len(found), found[:6])


def test_first_use_of_every_kernel_from_four_threads():
    """The four-thread run in a fresh process: the first launch of every kernel,
    and the call_once blocks of the hash launchers, raced from four threads."""
    out = subprocess.run([sys.executable, "-m", "tests.stream_feed"], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-2000:]
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report["launches"] == S.DECODERS * S.ROUNDS
    assert report["count"] == 0 and report["problems"] == [], report
