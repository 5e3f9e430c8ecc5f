"""The rc sort's speculative level 1 (csrc/boss_pipeline.hip: rc_level1_spec): the fused rc partition sizes
its level-1 buckets from the rc keys of every 8th canonical bucket instead of an exact histogram pass over
the whole canonical set, checks every run against its bucket's end and hands the rc sort a padded layout.
Bit-exact (W, last, F, the real-edge count) against the oracle, with the timings' rc_spec_l1 telling which
path ran: 1 the speculative buckets, 2 a bucket overflowed and the exact pass ran after it, 0 the exact pass
alone.

The path needs the canonical set left in its own speculative buckets, which the canonical sort does from 512
of its tiles (4.2 M k-mers) on: 300 000 of the bench generator's reads (36 M windows) for the main cases,
and tiled reads over a short genome, repeated up to 4.3 M windows, where the number of distinct k-mers is
what the case is about.  MTG_MSD_LEVELS=2 keeps both sorts at two levels on these sizes (the padded layout
is read by a level 2)."""
import importlib

import numpy as np
import pytest

import oracle_ctypes as O

import bench

boss = importlib.import_module("projects2014-metagenome_amd.boss")

pytestmark = pytest.mark.gpu

KB = 30  # BOSS k of the k = 31 graph: odd window length, u64 keys
TILE = 8192  # RcPartTraits<1>::TILE: canonical positions per workgroup of rc_partition_gapped_kernel


@pytest.fixture
def two_levels(monkeypatch):
    monkeypatch.setenv("MTG_MSD_LEVELS", "2")
    return monkeypatch


def _build(ctor, asc):
    n, L = asc.shape
    ctor.add_packed(asc.reshape(-1), np.arange(n + 1, dtype=np.uint64) * L)
    return ctor.build_chunk(), ctor.timings()


def _new_ctor():
    return boss.IBOSSChunkConstructor.initialize(KB, both_strands=True, bits_per_count=0, num_threads=8)


def _oracle(asc):
    return O.build_chunk(KB, [asc[i].tobytes() for i in range(len(asc))], canonical=True, bits_per_count=0)


def _assert_same(got, want, ctx):
    assert len(got.W) == len(want.W), ctx
    assert np.array_equal(got.W, want.W), ctx
    assert np.array_equal(got.last, want.last), ctx
    assert np.array_equal(got.F, want.F), ctx
    assert got.n_real == want.n_real, ctx


def _tiled(n_distinct, seed, min_windows=4_300_000, alphabet=b"ACGT"):
    """Reads of 150 tiling a random genome with exactly n_distinct windows of 31 (every window covered; the
    caller checks that they are distinct through the oracle's real-edge count), repeated to min_windows."""
    rng = np.random.default_rng(seed)
    G = n_distinct + KB
    genome = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=G)]
    starts = list(range(0, G - 150, 100)) + [G - 150]
    one = np.stack([genome[s:s + 150] for s in starts])
    reps = -(-min_windows // (len(starts) * 120))
    return np.ascontiguousarray(np.tile(one, (reps, 1)))


@pytest.fixture(scope="module")
def uniform():
    asc = bench.make_reads_host_codes(300_000, 150, 4711, "genome", 10.0)
    return asc, _oracle(asc)


def test_speculative_level1_uniform_reads(two_levels, uniform):
    asc, want = uniform
    got, t = _build(_new_ctor(), asc)
    print("rc_spec_l1", t.rc_spec_l1, "spec_levels", t.spec_levels, "fallbacks", t.spec_fallbacks, "U", t.n_unique)
    assert t.rc_spec_l1 == 1 and t.spec_fallbacks == 0, (t.rc_spec_l1, t.spec_fallbacks)
    _assert_same(got, want, "speculative rc level 1")


def test_forced_overflow_falls_back_to_exact_pass(two_levels, uniform):
    # buckets of half the sampled estimate (MTG_RC_SPEC=tiny) must overflow: the exact histogram pass and the
    # unchecked partition run after the refused one
    two_levels.setenv("MTG_RC_SPEC", "tiny")
    asc, want = uniform
    got, t = _build(_new_ctor(), asc)
    print("rc_spec_l1", t.rc_spec_l1, "fallbacks", t.spec_fallbacks)
    assert t.rc_spec_l1 == 2 and t.spec_fallbacks >= 1, (t.rc_spec_l1, t.spec_fallbacks)
    _assert_same(got, want, "speculative rc level 1, overflow")


def test_speculative_level1_off(two_levels, uniform):
    two_levels.setenv("MTG_RC_SPEC", "0")
    asc, want = uniform
    got, t = _build(_new_ctor(), asc)
    assert t.rc_spec_l1 == 0, t.rc_spec_l1
    _assert_same(got, want, "MTG_RC_SPEC=0")


@pytest.mark.parametrize("n_distinct", [TILE - 192, TILE + 1])
def test_tile_edges(two_levels, n_distinct):
    # the canonical set below one tile of the partition, and one key past a tile (a second workgroup with a
    # single position)
    asc = _tiled(n_distinct, 5)
    want = _oracle(asc)
    assert want.n_real == 2 * n_distinct  # odd window length: every canonical k-mer and its rc
    got, t = _build(_new_ctor(), asc)
    print("n_distinct", n_distinct, "rc_spec_l1", t.rc_spec_l1, "fallbacks", t.spec_fallbacks)
    assert t.n_unique == n_distinct
    assert t.rc_spec_l1 == 1 and t.spec_fallbacks == 0, (t.rc_spec_l1, t.spec_fallbacks)
    _assert_same(got, want, "%d distinct k-mers" % n_distinct)


def test_empty_last_canonical_buckets(two_levels):
    # a genome over A and C: every canonical k-mer is the forward one, so the canonical buckets of the upper
    # half of the key space are empty (the sample's last strides find nothing) while the rc keys, over G and
    # T, fill only the upper level-1 buckets
    asc = _tiled(40_000, 6, alphabet=b"AC")
    want = _oracle(asc)
    got, t = _build(_new_ctor(), asc)
    print("rc_spec_l1", t.rc_spec_l1, "fallbacks", t.spec_fallbacks, "U", t.n_unique)
    assert t.rc_spec_l1 == 1, (t.rc_spec_l1, t.spec_fallbacks)
    _assert_same(got, want, "two-letter genome")


def test_consecutive_builds_on_one_constructor(two_levels, uniform):
    # the step's scratch words (cursors, histograms, the overflow word) across builds on one constructor: a
    # smaller input after a larger one, then a build after one that overflowed
    asc, want = uniform
    small = np.ascontiguousarray(asc[:150_000])
    want_small = _oracle(small)
    ctor = _new_ctor()
    got, t = _build(ctor, asc)
    assert t.rc_spec_l1 == 1, t.rc_spec_l1
    _assert_same(got, want, "first build")
    got, t = _build(ctor, small)
    assert t.rc_spec_l1 == 1 and t.spec_fallbacks == 0, (t.rc_spec_l1, t.spec_fallbacks)
    _assert_same(got, want_small, "second, smaller build")
    two_levels.setenv("MTG_RC_SPEC", "tiny")
    over = _new_ctor()  # (the knobs are read when a constructor is made)
    got, t = _build(over, asc)
    assert t.rc_spec_l1 == 2, t.rc_spec_l1
    _assert_same(got, want, "the build that overflowed")
    got, t = _build(over, small)
    assert t.rc_spec_l1 == 2, t.rc_spec_l1
    _assert_same(got, want_small, "the build after it")
