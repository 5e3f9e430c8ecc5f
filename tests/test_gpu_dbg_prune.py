"""`concatenate --clear-dummy` on the device (mtg_boss_write_dbg_device_pruned, csrc/dbg_prune.hpp), its
erase step alone (mtg_boss_erase_edges_device) and the device-side Chunk::extend
(mtg_boss_chunk_extend_device).

Every file comparison is byte for byte against what `Chunk.write_dbg(..., prune=True)` (the host writer,
the specification) writes from the same arrays; n_valid must be equal and n_erased must be the input's
rows minus the host file's.  No tolerances.  The kernels' tile is 4096 rows (dbgdev::kTile)."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import oracle_ctypes as O
import seq_io
from test_dbg_io import _chunk
from test_gpu_dbg_device import DeviceArrays, _assert_same_files, _last, _symbols
from test_oracle_goldens import CONSTRUCT_SEQS
from test_suffix_route import (CHUNK_SEQS, concat_definition_rows, concat_oracle, pruned_definition,
                               random_reads)

boss = importlib.import_module("projects2014-metagenome_amd.boss")

pytestmark = pytest.mark.gpu

MTG_ERR_ARGUMENT = -5
TILE = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctor():
    """one constructor for the module: the entries use its mutex and stream, not its k"""
    return boss.IBOSSChunkConstructor.initialize(3)


def _prune_both(ctor, tmp_path, tag, ch, canonical, suffix_length=-1):
    """prunes and writes with both writers, compares bytes and counts; returns (n_valid, n_erased,
    device base, the host's file)"""
    hb, db = str(tmp_path / (tag + "_h")), str(tmp_path / (tag + "_d"))
    nv_h = ch.write_dbg(hb, canonical=canonical, mask_dummy=True, suffix_length=suffix_length, prune=True)
    host = boss.DbgFile(hb)
    with DeviceArrays() as dev:
        dc = dev.chunk(ch.k, ch.W, ch.last, ch.F)
        nv_d = ctor.write_dbg_device(dc, db, canonical=canonical, suffix_length=suffix_length, prune=True)
        t = ctor.last_dbg_timings
        assert t["device_ms"] > 0 and t["d2h_bytes"] > 0
        # the input arrays are only read
        W = np.empty(dc.n, np.uint8)
        last = np.empty(dc.n, np.uint8)
        assert boss.lib().mtg_memcpy_d2h(W.ctypes.data, dc.W, dc.n) == 0
        assert boss.lib().mtg_memcpy_d2h(last.ctypes.data, dc.last, dc.n) == 0
        assert np.array_equal(W, ch.W) and np.array_equal(last, ch.last), tag
    _assert_same_files(db, hb, tag)
    assert not os.path.exists(db + ".dbg.weights")
    assert nv_d == nv_h, tag
    assert ctor.last_dbg_erased == len(ch.W) - host.n, tag
    return nv_d, ctor.last_dbg_erased, db, host


# ------------------------------------------------------------ 1. concatenated suffix chunks

PRUNE_SEQS = CONSTRUCT_SEQS + random_reads(3, 30, 8, 40)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("k", [2, 3, 4, 7, 12, 20])
def test_concatenated_suffix_chunks(ctor, tmp_path, k, both):
    for L in range(1, min(k, 3)):
        cat = concat_oracle(k, PRUNE_SEQS, L, both)
        nv, n_erased, base, _ = _prune_both(ctor, tmp_path, "c%d_%d" % (k, L), cat, both)
        # the definition erases rows at these shapes (D.prune_rows): the kernels have work to do
        if k <= 7 or both:
            assert n_erased > 0, (k, L)
        f = boss.DbgFile(base)
        t, valid = pruned_definition(k, concat_definition_rows(k, PRUNE_SEQS, L, both))
        assert list(f.W) == t["W"] and list(f.last) == t["last"], (k, L)
        assert [int(x) for x in f.F] == t["F"], (k, L)
        assert list(f.valid) == valid and nv == f.n_valid == sum(valid), (k, L)


# ------------------------------------------------------------------- 2. nothing to prune

@pytest.mark.parametrize("k", [1, 3, 9])
def test_full_construction_has_nothing_to_prune(ctor, tmp_path, k):
    c = O.build_chunk(k, CONSTRUCT_SEQS, canonical=True)
    ch = boss.Chunk(k, np.asarray(c.W, np.uint8), np.asarray(c.last, np.uint8), np.asarray(c.F, np.uint64))
    nv, n_erased, base, _ = _prune_both(ctor, tmp_path, "f%d" % k, ch, True)
    assert n_erased == 0
    mb = str(tmp_path / "m")
    with DeviceArrays() as dev:
        dc = dev.chunk(k, ch.W, ch.last, ch.F)
        assert ctor.write_dbg_device(dc, mb, canonical=True, mask_dummy=True) == nv
    _assert_same_files(base, mb, "masked %d" % k)


def test_tiny_tables_and_a_table_without_roots(ctor, tmp_path):
    zero = np.zeros(5, np.uint64)
    one = boss.Chunk(3, np.zeros(1, np.uint8), np.zeros(1, np.uint8), zero)
    assert _prune_both(ctor, tmp_path, "one", one, False)[:2] == (0, 0)
    two = boss.Chunk(3, np.zeros(2, np.uint8), np.array([0, 1], np.uint8), np.ones(5, np.uint64))
    assert _prune_both(ctor, tmp_path, "two", two, False)[1] == 0
    # last[1] == 1: the main dummy node ends at row 1, so there are no roots and nothing is walked
    ch = _chunk(3, CONSTRUCT_SEQS)
    last = np.asarray(ch.last, np.uint8).copy()
    last[1] = 1
    ch = boss.Chunk(3, np.asarray(ch.W, np.uint8), last, np.asarray(ch.F, np.uint64))
    assert len(ch.W) > 2
    assert _prune_both(ctor, tmp_path, "noroots", ch, False, suffix_length=0)[1] == 0


# ------------------------------------------------------------------------------ 3. depth

@pytest.mark.parametrize("k", [30, 84])
def test_deep_trees(ctor, tmp_path, k):
    # k levels of the walk, a few hundred rows per level at the most.  Whatever the host erases here
    # (it may be nothing: _prune_both pins the count to the host's), every level is walked down and up.
    for L in (1, 2):
        cat = concat_oracle(k, CHUNK_SEQS, L, False)
        _prune_both(ctor, tmp_path, "d%d_%d" % (k, L), cat, False)


# ---------------------------------------------------------------------- 4. several tiles

def _erased_spans_tiles(F_in, F_out, n_in, n_out):
    """From the host's result alone: erased rows in two F intervals that lie at least one interval of
    >= TILE rows apart are more than TILE rows apart, so they fall into different tiles."""
    F_in = [int(x) for x in F_in] + [n_in - 1]
    F_out = [int(x) for x in F_out] + [n_out - 1]
    upto = [a - b for a, b in zip(F_in, F_out)]  # erased rows in [1, F[c]]
    inside = [upto[0]] + [upto[c + 1] - upto[c] for c in range(5)]  # in (F[c - 1], F[c]], c = 0..5
    for i in range(6):
        for j in range(i + 2, 6):
            if inside[i] > 0 and inside[j] > 0 and F_in[j - 1] - F_in[i] >= TILE:
                return True
    return False


@pytest.mark.parametrize("both,nodes", [(False, 591997), (True, 1159851)])
def test_transcripts_over_several_tiles(ctor, tmp_path, transcripts_1000, both, nodes):
    cat = concat_oracle(19, transcripts_1000, 1, both)
    nv, n_erased, _, host = _prune_both(ctor, tmp_path, "t", cat, both)
    assert nv == nodes
    assert n_erased > 0
    assert _erased_spans_tiles(cat.F, host.F, len(cat.W), host.n)


# ------------------------------------------------------------- 5. the erase step alone

def erase_edges_definition(W, last, F, erase):
    """dbg_io.hpp:262-300 (BOSS::erase_edges, boss.cpp:1342-1403) restated row by row"""
    W, last, erase = [int(x) for x in W], [int(x) for x in last], [int(x) for x in erase]
    out_W, out_last = [], []
    first_removed = [False] * 5
    for i in range(len(W)):
        c = W[i]
        if erase[i]:
            if c < 5:
                first_removed[c] = True
            if last[i] and len(out_W) > 1:
                out_last[-1] = 1
            continue
        out_W.append(c % 5 if c > 5 and first_removed[c % 5] else c)
        first_removed[c % 5] = False
        out_last.append(last[i])
    kept = np.concatenate([[0], np.cumsum(1 - np.asarray(erase[1:], np.int64))]) if len(W) > 1 else np.zeros(1, np.int64)
    out_F = [int(kept[int(f)]) for f in F]  # the kept rows in [1, F[c]]
    return np.array(out_W, np.uint8), np.array(out_last, np.uint8), out_F


def _erase_masks(rng, n, W, last):
    """(name, erase, last) cases; row 0 is never erased"""
    none = np.zeros(n, np.uint8)
    yield "none", none, last
    half = (rng.random(n) < 0.5).astype(np.uint8)
    half[0] = 0
    yield "half", half, last
    rest = np.zeros(n, np.uint8)
    rest[2:] = 1
    yield "from2", rest, last
    # one erased run over more than two tiles, `last` set only inside it, plain labels erased inside it:
    # the hand-over of `last` and the lost minus cross the tiles
    run = np.zeros(n, np.uint8)
    run[100:9000] = 1
    inside = np.zeros(n, np.uint8)
    inside[100:9000] = (rng.random(len(inside[100:9000])) < 0.3)
    yield "run", run, inside
    row1 = half.copy()
    if n > 1:
        row1[1] = 1
    yield "row1", row1, last


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 200003])
def test_erase_edges_alone(ctor, n):
    rng = np.random.default_rng(n)
    L = boss.lib()
    for density in ("p95", "sparse"):
        W = _symbols(rng, "boss_like", n)
        base_last = _last(rng, density, n)
        F = np.sort(rng.integers(0, n, size=5)).astype(np.uint64)
        for name, erase, last in _erase_masks(rng, n, W, base_last):
            want_W, want_last, want_F = erase_edges_definition(W, last, F, erase)
            with DeviceArrays() as dev:
                dc = dev.chunk(7, W, last, F)
                d_erase = dev.upload(erase)
                out = boss._DeviceChunk()
                out.W = dev.upload(np.full(n, 0xEE, np.uint8))
                out.last = dev.upload(np.full(n, 0xEE, np.uint8))
                ctor.erase_edges_device(dc, d_erase, out)
                ctx = (n, density, name)
                assert out.n == len(want_W) and out.k == 7, ctx
                assert [int(x) for x in out.F] == want_F, ctx
                got_W, got_last = np.empty(n, np.uint8), np.empty(n, np.uint8)
                in_W, in_last, in_erase = np.empty(n, np.uint8), np.empty(n, np.uint8), np.empty(n, np.uint8)
                for host, d in ((got_W, out.W), (got_last, out.last), (in_W, dc.W), (in_last, dc.last),
                                (in_erase, d_erase)):
                    assert L.mtg_memcpy_d2h(host.ctypes.data, d, n) == 0
                assert np.array_equal(got_W[:out.n], want_W), ctx
                assert np.array_equal(got_last[:out.n], want_last), ctx
                # nothing is written past the kept rows, and the input is only read
                assert np.all(got_W[out.n:] == 0xEE) and np.all(got_last[out.n:] == 0xEE), ctx
                assert np.array_equal(in_W, W) and np.array_equal(in_last, last), ctx
                assert np.array_equal(in_erase, erase), ctx


def test_erase_edges_refuses_row_0(ctor):
    with DeviceArrays() as dev:
        dc = dev.chunk(3, np.zeros(4, np.uint8), np.ones(4, np.uint8), np.zeros(5, np.uint64))
        out = boss._DeviceChunk()
        out.W = dev.upload(np.zeros(4, np.uint8))
        out.last = dev.upload(np.zeros(4, np.uint8))
        with pytest.raises(RuntimeError, match="row 0"):
            ctor.erase_edges_device(dc, dev.upload(np.array([1, 0, 0, 0], np.uint8)), out)


# -------------------------------------------------------- 6. mtg_boss_chunk_extend_device

def _download(dc, weighted):
    L = boss.lib()
    W, last = np.empty(dc.n, np.uint8), np.empty(dc.n, np.uint8)
    assert L.mtg_memcpy_d2h(W.ctypes.data, dc.W, dc.n) == 0
    assert L.mtg_memcpy_d2h(last.ctypes.data, dc.last, dc.n) == 0
    wts = None
    if weighted:
        wts = np.empty(dc.n, np.uint32)
        assert L.mtg_memcpy_d2h(wts.ctypes.data, dc.weights, 4 * dc.n) == 0
    return W, last, wts


@pytest.mark.parametrize("bits", [0, 8])
def test_extend_on_the_device_equals_concatenate(ctor, tmp_path, bits):
    k = 5
    chunks = []
    for suf in boss.generate_suffixes(1):
        c = O.build_suffix_chunk(k, PRUNE_SEQS, suf, True, bits)
        chunks.append(boss.Chunk(k, c.W, c.last, c.F, c.weights, n_real=0, n_dummy=0, bits_per_count=bits))
    want = boss.concatenate(chunks)
    rows = sum(len(c.W) for c in chunks)
    with DeviceArrays() as dev, boss.DeviceChunkBuffer(ctor, k, rows, weighted=bool(bits)) as buf:
        for c in chunks:
            buf.extend(dev.chunk(k, c.W, c.last, c.F, c.weights if bits else None))
        # a chunk of one row changes nothing
        n_before = buf.chunk.n
        buf.extend(dev.chunk(k, np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.zeros(5, np.uint64),
                             np.zeros(1, np.uint32) if bits else None))
        assert buf.chunk.n == n_before == len(want.W)
        W, last, wts = _download(buf.chunk, bool(bits))
        assert np.array_equal(W, want.W) and np.array_equal(last, want.last)
        assert [int(x) for x in buf.chunk.F] == [int(x) for x in want.F]
        if bits:
            assert np.array_equal(wts, want.weights)
        # the device-concatenated chunk through the pruned writer
        hb, db = str(tmp_path / "h"), str(tmp_path / "d")
        nv_h = want.write_dbg(hb, canonical=True, mask_dummy=True, prune=True)
        assert ctor.write_dbg_device(buf.chunk, db, canonical=True, prune=True) == nv_h
        _assert_same_files(db, hb)
        assert ctor.last_dbg_erased == len(want.W) - boss.DbgFile(hb).n > 0


def test_extend_refuses_mismatches(ctor):
    L = boss.lib()
    k = 5
    c = O.build_suffix_chunk(k, PRUNE_SEQS, "A", False, 8)
    with DeviceArrays() as dev, boss.DeviceChunkBuffer(ctor, k, 2 * len(c.W)) as buf:
        plain = dev.chunk(k, c.W, c.last, c.F)
        buf.extend(plain)
        n = buf.chunk.n
        with pytest.raises(RuntimeError, match="weighted and unweighted"):
            buf.extend(dev.chunk(k, c.W, c.last, c.F, c.weights))
        with pytest.raises(RuntimeError, match="incompatible"):
            buf.extend(dev.chunk(k + 1, c.W, c.last, c.F))
        buf.capacity = 2 * len(c.W) - 2  # one row short of a second copy's rows 1..
        rc = L.mtg_boss_chunk_extend_device(ctor._h, ctypes.byref(buf.chunk), buf.capacity, ctypes.byref(plain))
        assert rc == MTG_ERR_ARGUMENT and b"capacity" in L.mtg_last_error()
        assert buf.chunk.n == n and [int(x) for x in buf.chunk.F] == [int(x) for x in c.F]
        buf.capacity += 1
        buf.extend(plain)
        assert buf.chunk.n == 2 * len(c.W) - 1


# ------------------------------------------------- 7. the builder's own chunks, end to end

def test_builders_suffix_chunks_end_to_end(tmp_path):
    k = 11
    seqs = seq_io.read_sequences(os.path.join(GOLDEN, "transcripts_100.fa"))
    data = b"".join((s if isinstance(s, bytes) else s.encode()) + b"$" for s in seqs)
    host_chunks = []
    for suf in boss.generate_suffixes(1):
        c = boss.IBOSSChunkConstructor.initialize(k, filter_suffix=suf)
        c.add_sequences(seqs)
        host_chunks.append(c.build_chunk())
    cat = boss.concatenate(host_chunks)
    hb, db = str(tmp_path / "h"), str(tmp_path / "d")
    nv_h = cat.write_dbg(hb, mask_dummy=True, prune=True)
    writer = boss.IBOSSChunkConstructor.initialize(k)
    with DeviceArrays() as dev, boss.DeviceChunkBuffer(writer, k, len(cat.W)) as buf:
        d = dev.upload(np.frombuffer(data, np.uint8))
        for suf in boss.generate_suffixes(1):
            c = boss.IBOSSChunkConstructor.initialize(k, filter_suffix=suf)
            dc = c.build_device(d, len(data))
            buf.extend(dc)
        assert buf.chunk.n == len(cat.W)
        assert writer.write_dbg_device(buf.chunk, db, prune=True) == nv_h
    _assert_same_files(db, hb)
    assert writer.last_dbg_erased == len(cat.W) - boss.DbgFile(hb).n
