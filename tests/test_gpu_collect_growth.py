"""The batched collects' growing sorted set (collect_stage.hpp: AppendSet) grown after its first fill.

Every bounded-memory collect appends its slices' distinct k-mers to one set, sized from the first slice's
distinct ratio (+25 %).  Random reads keep that ratio representative, so no other test makes the set grow
a second time (Workspace::get with `keep`: a larger buffer, the appended keys copied over).  Here half of
all windows are the one k-mer A...A, which sits in the first top-char bin (and the first level-1 bucket):
the first balanced slice is almost all duplicates, its ratio sizes the set far below what the next slices
append, and the set grows with kept contents.  In canonical mode the T...T side mirrors it in the last
bin.  (The key ranges of this input by the collect's own arithmetic: basic mode, 3 ranges of 58 / 6942 /
13893 distinct k-mers, the set sized 202, then 8750, then 26116; canonical mode, 5813 / 22839 / 5644,
sized 27525, then 35815.)  Every route is bit-exact against the oracle on the same reads."""
import functools
import importlib

import pytest

import oracle_ctypes as O
from test_gpu_dist import dist_chunks
from test_gpu_parity import _random_reads, assert_same

boss = importlib.import_module("projects2014-metagenome_amd.boss")

pytestmark = pytest.mark.gpu

K_BOSS = 15  # K = 16 > RB_CHARS + 2: every batched route applies
READS = [b"A" * 100] * 300 + _random_reads(777, 300, 100, 30000)


@functools.lru_cache(maxsize=None)
def _want(canonical, bits):
    return O.build_chunk(K_BOSS, READS, canonical=canonical, bits_per_count=bits)


def _check(canonical, bits):
    ctor = boss.IBOSSChunkConstructor.initialize(K_BOSS, both_strands=canonical, bits_per_count=bits)
    ctor.add_sequences(READS)
    got = ctor.build_chunk()
    assert_same(got, _want(canonical, bits), "canonical=%s bits=%d" % (canonical, bits))
    return ctor.timings()


def _first_bin_kmers(canonical):
    # distinct real k-mers (K chars) of the first top-char bin: the node's last RB_CHARS = 4 chars are A
    K = K_BOSS + 1
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    kmers = set()
    for r in set(READS):
        for s in (r, r.translate(comp)[::-1]) if canonical else (r,):
            kmers.update(s[i:i + K] for i in range(len(s) - K + 1))
    return sum(1 for x in kmers if x[K - 5:K - 1] == b"AAAA")


@pytest.mark.parametrize("canonical", [False, True])
def test_first_slice_cannot_size_the_set(canonical):
    # the input's premise (no GPU needed): the real edges are more than 4x the first bin's distinct k-mers,
    # so an estimate from the first slice cannot cover the whole set
    assert _want(canonical, 0).n_real > 4 * _first_bin_kmers(canonical)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("bits", [0, 8])
def test_growth_key_ranges(monkeypatch, bits, canonical):
    monkeypatch.setenv("MTG_COLLECT", "ranges")
    monkeypatch.setenv("MTG_RANGES", "3")
    t = _check(canonical, bits)
    assert t.collect_mode == 1 and t.n_batches == 3, (t.collect_mode, t.n_batches)


@pytest.mark.parametrize("canonical", [False, True])
def test_growth_fused_rounds_counted(monkeypatch, canonical):
    # the counted rounds reserve nothing up front: the set starts at cap = 0
    monkeypatch.setenv("MTG_FUSED_MIN", "0")
    monkeypatch.setenv("MTG_RANGES", "3")
    t = _check(canonical, 8)
    assert t.collect_mode == 2 and t.n_batches == 3, (t.collect_mode, t.n_batches)


@pytest.mark.parametrize("collect", ["ranges", "routed"])
def test_growth_two_ranks(monkeypatch, collect):
    # collect_ranges_dist, and the routed rounds of dist_collect_routed
    monkeypatch.setenv("MTG_RANGES", "3")
    if collect == "ranges":
        monkeypatch.setenv("MTG_COLLECT", "ranges")
    ctors = []
    chunks = dist_chunks(K_BOSS, [READS[0::2], READS[1::2]], True, 8, ctors_out=ctors)
    assert_same(boss.concatenate(chunks), _want(True, 8), "two ranks, %s" % collect)
    mode = 2 if collect == "routed" else 1
    assert all(c.timings().collect_mode == mode and c.timings().n_batches == 3 for c in ctors)


def test_growth_spill_skewed_slice(monkeypatch):
    # no growing set in the spilled build: the shared range step on a slice that is one k-mer
    monkeypatch.setenv("MTG_SPILL", "1")
    monkeypatch.setenv("MTG_RANGES", "3")
    t = _check(True, 8)
    assert t.spilled_bytes > 0 and t.n_batches == 3
