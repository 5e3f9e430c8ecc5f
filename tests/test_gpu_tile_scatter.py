"""The tile bucket-scatter the five partition kernels share (csrc/tile_scatter.hpp) on bucket shapes the
other suites' random reads do not force: reads over two letters only, so most level-1 buckets of a tile
are empty and a few hold most of it, with a ragged last tile.  Bit-exact against the oracle; every case
runs the fused K1 on small inputs (MTG_FUSED_MIN=0)."""
import numpy as np
import pytest

import bench

from test_gpu_parity import _random_reads, check
from test_gpu_rounds import ROUNDS, _check

pytestmark = pytest.mark.gpu

AC = bytes.maketrans(b"ACGTacgt", b"ACACacac")
GT = bytes.maketrans(b"ACGTacgt", b"GTGTgtgt")

# 230 reads of 150 chars: 34 730 chars with the read separators, 4.2 of pass B's 8192-window tiles (u64
# keys) and 8.5 of its 4096-window tiles (u128), the last one ragged in both.  The plan of an input this
# small has one level of 2 or 3 bits (4 or 8 level-1 buckets, the two-letter keys in one or two of them);
# the NB = 1024 case repeats the reads for a wider plan.  A one-off kernel trace of this file showed
# extract_partition_fast_kernel<512, 512, 0, -1> (5 launches: the small uncounted u64 cases),
# <512, 1024, 0, -1> (1: the NB = 1024 case) and <512, 512, 31, 1> (1: the 300 000-read canonical case),
# extract_partition_kernel<1, true, 512, 0> (1: k = 20 with counts), extract_partition_fast2_kernel<512, 0, 8>
# (3: the k = 63 rounds), msd_partition_kernel<1, false> (8) and <2, false> (3), and no launch of
# rc_partition_gapped_kernel (see test_skewed_canonical_rc_fuse).
N_READS = 230


@pytest.fixture(scope="module")
def skewed():
    # a genome over A and C, then one over G and T (N and lower case kept)
    reads = _random_reads(97, N_READS, 150, 4000, n_rate=0.002, lower=True)
    return [r.translate(AC if i < N_READS // 2 else GT) for i, r in enumerate(reads)]


@pytest.fixture
def small_fused(monkeypatch):
    monkeypatch.setenv("MTG_FUSED_MIN", "0")
    return monkeypatch


@pytest.mark.parametrize("k,bits", [(20, 0), (31, 0), (20, 8), (63, 0)])
def test_skewed_buckets(small_fused, skewed, k, bits):
    # u64 uncounted (the fast kernel) and the generic counted kernel; the fused K1 takes u64 keys only, so
    # the plain k = 63 build scatters its u128 keys with msd_partition_kernel<2> alone (the u128 pass B,
    # the fast2 kernel, runs in test_skewed_rounds)
    check(k, skewed, False, bits)


def test_skewed_buckets_1024(small_fused, skewed):
    # NB = 1024, two buckets a thread.  MTG_FUSED_B1 is capped by the plan's width: 9 bits at 3.0 M windows
    # (the reads 120 times), so the reads are repeated 250 times (6.3 M windows, 773 tiles); nearly all of
    # a tile's buckets are empty
    small_fused.setenv("MTG_FUSED_B1", "10")
    check(31, skewed * 250, False, 0)


@pytest.mark.parametrize("one_b", ["1", "0"])
@pytest.mark.parametrize("k", [31, 63])
def test_skewed_rounds(small_fused, skewed, k, one_b):
    # one round's mask selects few or none of a tile's keys: whole tiles stage nothing
    small_fused.setenv("MTG_RANGES", "2")
    small_fused.setenv("MTG_ROUNDS_ONE_B", one_b)
    _, t = _check(k, skewed, True, 0)
    assert t.collect_mode == ROUNDS and t.n_batches == 2, (t.collect_mode, t.n_batches)


def test_skewed_canonical_rc_fuse(small_fused):
    # The canonical set at an odd window length (BOSS k = 30, the k = 31 graph) and at the size where the
    # rc stage can read it in its speculative buckets (a sort input of 512 tiles or more): 300 000 of the
    # bench generator's reads (36 M windows), the first half over A and C, the second over G and T.
    # Checked once by hand: on this skew the speculative buckets, sized from a sample, overflow
    # (timings: spec_levels = 0, spec_fallbacks = 1), the shared scatter raises its overflow word and the
    # build runs the exact levels instead, so rc_partition_gapped_kernel (MTG_RC_FUSE at its default)
    # does NOT run here.  Its fallback search before the shared scatter is left to the unskewed reads of
    # test_gpu_scale.py (test_bench_generator_2m_reads_k31, test_bench_generator_speculative_fallbacks).
    asc = bench.make_reads_host_codes(300_000, 150, 97, "genome", 10.0)
    half = len(asc) // 2
    asc = np.concatenate([np.frombuffer(AC, np.uint8)[asc[:half]], np.frombuffer(GT, np.uint8)[asc[half:]]])
    check(30, [r.tobytes() for r in asc], True, 0)
