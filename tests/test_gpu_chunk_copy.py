"""A chunk's way off the device (chunk_host.hpp): W crosses PCIe as 4-bit codes and narrow weights as 1 or 2
bytes, in pieces that host threads unpack as they land.  By default only arrays of 128 Mi rows take that
path; MTG_D2H_PIECE=<bytes> sends arrays of any size through it, so its edges -- more pieces than threads,
a short last piece, the half-filled last byte of an odd row count -- are checked here on a few thousand
rows.  Also: the rows of a spilled build belong to that build, and nothing of them reaches the next one."""
import functools
import importlib

import numpy as np
import pytest

import oracle_ctypes as O
from test_gpu_dbg_device import _readback
from test_gpu_parity import assert_same

boss = importlib.import_module("projects2014-metagenome_amd.boss")

pytestmark = pytest.mark.gpu

K = 12
PIECE = 64  # packed bytes per piece: 128 W rows


@functools.lru_cache(maxsize=None)
def _oracle(reads, canonical, bits):
    return O.build_chunk(K, list(reads), canonical=canonical, bits_per_count=bits)


def _prefixes(seqs, canonical):
    """Two prefixes of the read list whose row counts differ in parity: the whole list, and the longest
    shorter prefix where the parity of n has flipped."""
    whole = tuple(seqs)
    n0 = len(_oracle(whole, canonical, 0).W)
    for m in range(len(whole) - 1, 0, -1):
        if (len(_oracle(whole[:m], canonical, 0).W) - n0) % 2:
            return whole, whole[:m]
    raise AssertionError("no prefix flips the parity of the row count")


def _gpu_chunk(reads, canonical, bits):
    ctor = boss.IBOSSChunkConstructor.initialize(K, both_strands=canonical, bits_per_count=bits, num_threads=2)
    ctor.add_sequences(list(reads))
    return ctor.build_chunk()


@pytest.mark.parametrize("bits", [0, 8, 16, 32])
@pytest.mark.parametrize("canonical", [True, False])
def test_piece_copy_small(monkeypatch, transcripts_1000, canonical, bits):
    parities = set()
    for reads in _prefixes(transcripts_1000[:300], canonical):
        want = _oracle(reads, canonical, bits)
        n = len(want.W)
        assert n > 4 * 128  # several pieces of 128 rows for both threads, and a short last one
        parities.add(n % 2)
        monkeypatch.delenv("MTG_D2H_PIECE", raising=False)
        plain = _gpu_chunk(reads, canonical, bits)
        monkeypatch.setenv("MTG_D2H_PIECE", str(PIECE))  # read when the constructor is made
        got = _gpu_chunk(reads, canonical, bits)
        ctx = "canonical=%s bits=%d n=%d" % (canonical, bits, n)
        assert_same(got, want, "pieces, " + ctx)
        assert_same(plain, want, "plain, " + ctx)
        assert_same(got, plain, "pieces against plain, " + ctx)
    assert parities == {0, 1}  # the odd n's last packed byte holds one W value


def test_spill_rows_owned_by_build(monkeypatch, transcripts_1000):
    monkeypatch.setenv("MTG_SPILL", "1")
    monkeypatch.setenv("MTG_RANGES", "3")
    reads = tuple(transcripts_1000[:300])
    want = _oracle(reads, True, 8)
    fewer = _oracle(reads[:150], True, 8)
    ctor = boss.IBOSSChunkConstructor.initialize(K, both_strands=True, bits_per_count=8)
    for batch, expect in ((reads, want), (reads[:150], fewer)):
        ctor.add_sequences(list(batch))
        got = ctor.build_chunk()
        assert ctor.timings().spilled_bytes > 0
        assert_same(got, expect, "spilled build of %d reads" % len(batch))
    # a device build on the same constructor: in HBM, with nothing of the spilled builds in it
    data = b"".join((s if isinstance(s, bytes) else s.encode()) + b"$" for s in reads)
    L = boss.lib()
    d = L.mtg_device_alloc(0, len(data))
    try:
        assert L.mtg_memcpy_h2d(d, data, len(data)) == 0
        dc = ctor.build_device(d, len(data))
        assert ctor.timings().spilled_bytes == 0
        W, last, wts = _readback(dc)
        assert dc.n == len(want.W) and list(dc.F) == [int(x) for x in want.F]
        assert np.array_equal(W, want.W) and np.array_equal(last, want.last)
        assert np.array_equal(wts, want.weights)
    finally:
        L.mtg_device_free(d)
