"""Unitigs with k-mer counts from the device chunk (mtg_boss_unitigs_device, csrc/unitigs.hpp).

Two exact checks, no tolerances.  Against the definition (tests/unitigs_definition.py): sequences, counts,
order and the written files' bytes.  Round trip: the unitigs rebuilt with their counts, on the device and
through the files, give the source chunk bit for bit.  The cleaning filters must reproduce the four goldens
of the reference's integration_tests/test_clean.py on transcripts_1000.fa.  The kernels' tile is 4096 rows
and the ranking doubles per round, so the cases hold a unitig longer than four tiles (more than 14 rounds)
and closed chains of 5, 4097 and 9000 k-mers."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import oracle_ctypes as O
import unitigs_definition as U
from test_gpu_dbg_device import DeviceArrays
from test_gpu_parity import assert_same
from test_unitigs_definition import GOLDENS

boss = importlib.import_module("projects2014-metagenome_amd.boss")

pytestmark = pytest.mark.gpu

MTG_ERR_ARGUMENT = -5


def _random_reads(seed, n, length, genome_len):
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), size=genome_len))
    return [genome[s:s + length] for s in rng.integers(0, genome_len - length, size=n)]


def _random_seq(seed, n):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), size=n))


def _closed(seed, L, K):
    s = _random_seq(seed, L)
    return (s * (1 + (L + K) // L))[:L + K - 1]


# name -> (K, sequences, canonical, count width)
GRAPHS = {
    "fork_join": (4, ["GGAACGTTAGG", "TCCACGTTCTT", "GGAACGTTAGG"], False, 8),
    "tip": (4, ["AACCGGTTAC", "CCGGA"], False, 8),
    "closed_chain": (5, ["ACGGTCATTG" + "ACGG"], False, 8),
    "self_loop": (4, ["A" * 9, "CCGTA"], False, 8),
    "palindrome": (4, ["ACGT", "GGACGTCC"], True, 8),
    "isolated": (6, ["ACGGTC", "TTTTTTTTGA"], False, 8),
    "dense_k3": (3, _random_reads(3, 40, 30, 400), False, 8),
    "dense_k4": (4, _random_reads(4, 60, 30, 600), True, 8),
    "dense_k5": (5, _random_reads(5, 200, 40, 3000), False, 4),
    "k21": (21, _random_reads(21, 300, 100, 5000), False, 8),
    "k21_canonical": (21, _random_reads(22, 300, 100, 5000), True, 8),
    "long_unitig": (25, [_random_seq(7, 20000)], False, 8),
    "closed_chains": (25, [_closed(11, 5, 25), _closed(12, 4097, 25), _closed(13, 9000, 25)] +
                      _random_reads(14, 50, 100, 2000), False, 8),
    "k85": (85, _random_reads(85, 100, 200, 3000), False, 8),
    "no_real_edge": (5, ["ACG", "NNNNNNNN"], False, 8),
    "one_kmer": (5, ["ACGGT"], False, 8),
    "unweighted": (21, _random_reads(23, 300, 100, 5000), True, 0),
}


def _readback(dc, weighted):
    L = boss.lib()
    W, last = np.empty(dc.n, np.uint8), np.empty(dc.n, np.uint8)
    assert L.mtg_memcpy_d2h(W.ctypes.data, dc.W, dc.n) == 0
    assert L.mtg_memcpy_d2h(last.ctypes.data, dc.last, dc.n) == 0
    wts = None
    if weighted:
        wts = np.empty(dc.n, np.uint32)
        assert L.mtg_memcpy_d2h(wts.ctypes.data, dc.weights, 4 * dc.n) == 0
    return boss.Chunk(dc.k, W, last, np.array(list(dc.F), np.uint64), wts, dc.n_real, dc.n_dummy)


def _fetch(ptr, count, dtype):
    a = np.empty(count, dtype)
    if count:
        assert boss.lib().mtg_memcpy_d2h(a.ctypes.data, ptr, a.nbytes) == 0
    return a


class Source:
    """a graph built on the device; the chunk lives as long as its constructor builds nothing else"""

    def __init__(self, dev, K, seqs, canonical, bits):
        self.K, self.bits = K, bits
        data = b"".join((s if isinstance(s, bytes) else s.encode()) + b"$" for s in seqs)
        self.d, self.len = dev.upload(np.frombuffer(data, np.uint8)), len(data)
        self.ctor = boss.IBOSSChunkConstructor.initialize(K - 1, both_strands=canonical, bits_per_count=bits)
        self.dc = self.ctor.build_device(self.d, self.len)
        self.chunk = _readback(self.dc, bool(bits))


def _check_against_definition(src, want, tmp_path, params=(1, 1)):
    """device arrays and files == the definition's records; returns the DeviceUnitigs"""
    weighted = bool(src.bits)
    u = src.ctor.unitigs_device(src.dc, *params)
    seq, starts, counts = U.device_layout(src.K, want["records"], weighted)
    assert (u.n_records, u.seq_len) == (len(want["records"]), len(seq))
    assert (u.n_dropped_records, u.n_dropped_kmers) == (want["dropped_records"], want["dropped_kmers"])
    assert _fetch(u.seq, u.seq_len, np.uint8).tobytes() == seq
    assert np.array_equal(_fetch(u.record_starts, u.n_records + 1, np.uint64), starts)
    if weighted:
        assert u.n_kmers == len(counts)
        assert np.array_equal(_fetch(u.kmer_counts, u.n_kmers, np.uint32), counts)
    else:
        assert not u.kmer_counts
    base = str(tmp_path / "u")
    stats = src.ctor.write_unitigs_device(src.dc, base + ".fasta.gz", *params)
    assert stats["n_records"] == u.n_records and stats["n_kmers"] == u.n_kmers
    assert stats["n_dropped_kmers"] == u.n_dropped_kmers
    fasta, kc = U.file_payloads(src.K, want["records"], weighted)
    assert U.read_gz(base + ".fasta.gz") == fasta
    assert sorted(os.listdir(str(tmp_path))) == ["u.fasta.gz"] + (["u.kmer_counts.gz"] if weighted else [])
    if weighted:
        assert U.read_gz(base + ".kmer_counts.gz") == kc
    return u, base


def _rebuild_device(u, K, bits):
    ctor = boss.IBOSSChunkConstructor.initialize(K - 1, both_strands=False, bits_per_count=bits)
    runs = ctor.kmer_counts_to_reads(*u.counts_args()) if bits and u.n_records else None
    return _readback(ctor.build_device(*u.build_args(runs)), bool(bits))


def _rebuild_files(base, K, bits):
    ctor = boss.IBOSSChunkConstructor.initialize(K - 1, both_strands=False, bits_per_count=bits)
    if bits:
        ctor.add_fasta_counts(base)
    else:
        ctor.add_fasta(base + ".fasta.gz")
    return ctor.build_chunk()


def _round_trip(src, u, base, tag):
    assert_same(_rebuild_device(u, src.K, src.bits), src.chunk, tag + " device")
    assert_same(_rebuild_files(base, src.K, src.bits), src.chunk, tag + " files")


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_definition_and_round_trip(tmp_path, name):
    K, seqs, canonical, bits = GRAPHS[name]
    cnt = U.count_kmers(K, seqs, canonical, bits)
    want = U.unitigs(K, cnt)
    with DeviceArrays() as dev:
        src = Source(dev, K, seqs, canonical, bits)
        assert src.dc.n_real == len(cnt)
        u, base = _check_against_definition(src, want, tmp_path)
        assert u.n_kmers == len(cnt)
        rounds = src.ctor.unitigs_last_rounds()
        print(name, "rows", src.dc.n, "records", u.n_records, "ranking rounds", rounds)
        if name == "long_unitig":
            assert max(len(w) for _, w in want["records"]) > 4 * 4096 and rounds > 14
        if name == "closed_chains":
            assert {5, 4097, 9000} <= {len(w) for _, w in want["records"]}
        if name == "no_real_edge":
            assert u.n_records == 0 and U.read_gz(base + ".kmer_counts.gz") == b"\x05\x00\x00\x00"
        _round_trip(src, u, base, name)


@pytest.mark.parametrize("name", ["tip", "isolated", "self_loop", "dense_k5", "k21_canonical", "closed_chains"])
@pytest.mark.parametrize("params", [(3, 1), (1, 2), (30, 2)])
def test_filters_against_definition(tmp_path, name, params):
    K, seqs, canonical, bits = GRAPHS[name]
    cnt = U.count_kmers(K, seqs, canonical, bits)
    with DeviceArrays() as dev:
        src = Source(dev, K, seqs, canonical, bits)
        _check_against_definition(src, U.unitigs(K, cnt, *params), tmp_path, params)


@pytest.mark.parametrize("K,canonical,bits", [(20, False, 8), (20, False, 2), (31, True, 8)])
def test_transcripts_round_trip(tmp_path, transcripts_1000, K, canonical, bits):
    with DeviceArrays() as dev:
        src = Source(dev, K, transcripts_1000, canonical, bits)
        u = src.ctor.unitigs_device(src.dc)
        assert u.n_kmers == src.dc.n_real and u.n_dropped_kmers == 0
        base = str(tmp_path / "t")
        src.ctor.write_unitigs_device(src.dc, base)
        _round_trip(src, u, base, "transcripts K=%d" % K)


@pytest.fixture(scope="module")
def transcripts_chains(transcripts_1000):
    cnt = U.count_kmers(20, transcripts_1000, False, 8)
    return cnt, U.all_chains(20, cnt)


@pytest.mark.parametrize("params,kmers_left,avg", GOLDENS)
def test_cleaning_goldens(tmp_path, transcripts_1000, transcripts_chains, params, kmers_left, avg):
    K = 20
    cnt, chains = transcripts_chains
    want = U.unitigs(K, cnt, *params, chains=chains)
    with DeviceArrays() as dev:
        src = Source(dev, K, transcripts_1000, False, 8)
        u = src.ctor.unitigs_device(src.dc, *params)
        assert (u.n_dropped_records, u.n_dropped_kmers) == (want["dropped_records"], want["dropped_kmers"])
        assert u.n_records == len(want["records"])
        ctor = boss.IBOSSChunkConstructor.initialize(K - 1, bits_per_count=8)
        runs = ctor.kmer_counts_to_reads(*u.counts_args())
        dc = ctor.build_device(*u.build_args(runs))
        n_valid = ctor.write_dbg_device(dc, str(tmp_path / "clean"), mask_dummy=True)
        w = _readback(dc, True).weights.astype(np.float64)
        print("params", params, "n_valid", n_valid, "avg", "{:.6g}".format(w.sum() / np.count_nonzero(w)))
        assert n_valid == kmers_left
        assert "{:.6g}".format(w.sum() / np.count_nonzero(w)) == avg


def test_source_chunk_is_intact_and_next_build_is_exact(tmp_path, transcripts_1000):
    K = 20
    want = O.build_chunk(K - 1, transcripts_1000, canonical=False, bits_per_count=8)
    with DeviceArrays() as dev:
        src = Source(dev, K, transcripts_1000, False, 8)
        assert_same(src.chunk, want, "source")
        src.ctor.unitigs_device(src.dc, 60, 3)
        src.ctor.write_unitigs_device(src.dc, str(tmp_path / "c"), 60, 3)
        after = _readback(src.dc, True)
        assert_same(after, want, "after the extraction")
        assert list(src.dc.F) == [int(x) for x in want.F]
        again = _readback(src.ctor.build_device(src.d, src.len), True)
        assert_same(again, want, "next build")


def test_errors(tmp_path):
    L = boss.lib()
    K, seqs, canonical, _ = GRAPHS["k21"]
    with DeviceArrays() as dev:
        src = Source(dev, K, seqs, canonical, 0)
        p = boss._UnitigParams(1, 2)
        out = boss._DeviceUnitigs()
        rc = L.mtg_boss_unitigs_device(src.ctor._h, ctypes.byref(src.dc), ctypes.byref(p), None, ctypes.byref(out))
        assert rc == MTG_ERR_ARGUMENT and b"weights" in L.mtg_last_error()
        with pytest.raises(RuntimeError, match="weights"):
            src.ctor.write_unitigs_device(src.dc, str(tmp_path / "a"), 1, 2)
        assert os.listdir(str(tmp_path)) == []
        weighted = Source(dev, K, seqs, canonical, 8)
        with pytest.raises(RuntimeError, match="Can't write"):
            weighted.ctor.write_unitigs_device(weighted.dc, str(tmp_path / "missing" / "a"))
        assert os.listdir(str(tmp_path)) == []
        # the constructor works after the failed call
        assert weighted.ctor.write_unitigs_device(weighted.dc, str(tmp_path / "b"))["n_kmers"] == weighted.dc.n_real
