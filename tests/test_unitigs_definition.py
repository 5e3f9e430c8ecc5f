"""The definition of unitigs and of the two cleaning filters (tests/unitigs_definition.py), checked
against the reference's own numbers and on hand-made graphs.  No device: this pins the specification the
GPU tests compare mtg_boss_unitigs_device with.

The goldens are those of the reference's integration_tests/test_clean.py for transcripts_1000.fa at
K = 20, basic mode, count width 8: the k-mers left after cleaning and their average weight printed with
six significant digits."""
import pytest

import unitigs_definition as U

K = 20
GOLDENS = [((1, 1), 591997, "2.48587"),
           ((60, 1), 589774, "2.49001"),
           ((1, 3), 167395, "5.52732"),
           ((60, 3), 167224, "5.52757")]


@pytest.fixture(scope="module")
def transcripts_kmers(transcripts_1000):
    cnt = U.count_kmers(K, transcripts_1000, False, 8)
    return cnt, U.all_chains(K, cnt)


@pytest.mark.parametrize("params,kmers_left,avg", GOLDENS)
def test_reference_goldens(transcripts_kmers, params, kmers_left, avg):
    transcripts_kmers, chains = transcripts_kmers
    r = U.unitigs(K, transcripts_kmers, *params, chains=chains)
    weights = [x for _, w in r["records"] for x in w]
    print("params", params, "k-mers left", len(weights), "avg", "{:.6g}".format(sum(weights) / len(weights)))
    assert len(weights) == kmers_left
    assert "{:.6g}".format(sum(weights) / len(weights)) == avg
    assert len(weights) + r["dropped_kmers"] == len(transcripts_kmers)
    assert all(len(s) == len(w) + K - 1 for s, w in r["records"])


def _seqs(K, seqs, **kw):
    cnt = U.count_kmers(K, seqs, kw.pop("canonical", False), 8)
    return cnt, U.unitigs(K, cnt, **kw)


def _covers_once(K, cnt, records):
    seen = [s[i:i + K] for s, _ in records for i in range(len(s) - K + 1)]
    assert sorted(seen) == sorted(cnt)
    for s, w in records:
        assert w == [cnt[s[i:i + K]] for i in range(len(s) - K + 1)]


def test_fork_and_join():
    # two paths that share their middle: ...AAC>G<TTA... and ...CAC>G<TTC...: the shared k-mers form one unitig
    K = 4
    a, b = "GGAACGTTAGG", "TCCACGTTCTT"
    cnt, r = _seqs(K, [a, b])
    _covers_once(K, cnt, r["records"])
    seqs = [s for s, _ in r["records"]]
    assert "ACGTT" in seqs  # ACGT -> CGTT: joined before (AACG, CACG), forked after (GTTA, GTTC)
    for s in seqs:
        for i in range(len(s) - K):
            u, v = s[i:i + K], s[i + 1:i + 1 + K]
            assert sum(u[1:] + c in cnt for c in "ACGT") == 1 and sum(c + v[:-1] in cnt for c in "ACGT") == 1
    assert r["dropped_records"] == 0


def test_tips_are_dropped_and_bridges_kept():
    K = 4
    main = "AACCGGTTAC"
    tip = "CCGGA"  # leaves the main path after CCGG and dead-ends
    cnt, r = _seqs(K, [main, tip], min_tip_size=1)
    _covers_once(K, cnt, r["records"])
    _, r3 = _seqs(K, [main, tip], min_tip_size=3)
    kept = {s[i:i + K] for s, _ in r3["records"] for i in range(len(s) - K + 1)}
    assert "CGGA" not in kept  # one k-mer, no successor, one predecessor: a sink tip
    assert "CGGT" not in kept or len([s for s, _ in r3["records"] if "CGGT" in s][0]) >= K + 2
    assert r3["dropped_records"] >= 1 and r3["dropped_kmers"] == len(cnt) - len(kept)


def test_closed_chain_starts_at_its_smallest_row():
    K = 5
    s = "ACGGTCATTG"
    cnt, r = _seqs(K, [s + s[:K - 1]])
    assert len(cnt) == len(s)
    assert len(r["records"]) == 1
    seq, w = r["records"][0]
    assert len(w) == len(s) and seq[:K] == U.boss_order(K, cnt)[0]
    _covers_once(K, cnt, r["records"])


def test_self_loop():
    K = 4
    cnt, r = _seqs(K, ["A" * 9])
    assert cnt == {"AAAA": 6}
    assert r["records"] == [("AAAA", [6])]
    # a tip filter sees one predecessor and one successor (itself): kept
    assert U.unitigs(K, cnt, 5, 1)["records"] == [("AAAA", [6])]


def test_palindromic_kmer_in_canonical_mode():
    K = 4
    cnt, r = _seqs(K, ["ACGT"], canonical=True)
    assert cnt == {"ACGT": 2}
    assert r["records"] == [("ACGT", [2])]


def test_isolated_kmer_is_a_tip():
    K = 4
    cnt = U.count_kmers(K, ["ACGG"], False, 8)
    assert U.unitigs(K, cnt)["records"] == [("ACGG", [1])]
    r = U.unitigs(K, cnt, 2, 1)
    assert r["records"] == [] and (r["dropped_records"], r["dropped_kmers"]) == (1, 1)


def test_median_abundance():
    K = 4
    cnt, r = _seqs(K, ["ACGGTC", "ACGGTC", "ACGGTC", "TTTTG"], min_median_abundance=2)
    assert [s for s, _ in r["records"]] == ["ACGGTC"]
    # TTTT precedes itself and TTTG: two unitigs of one weak k-mer each
    assert (r["dropped_records"], r["dropped_kmers"]) == (2, 2)
