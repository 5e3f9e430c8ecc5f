"""TEST INFRASTRUCTURE ONLY -- the unitigs of a de Bruijn graph with their k-mer counts, from the
definition over strings (no BOSS table, no navigation), for the tests of mtg_boss_unitigs_device.

A k-mer is a string of K chars over ACGT with a count.  k-mer u precedes v when u[1:] == v[:-1]; indeg
and outdeg count k-mers.  u -> v is a link iff outdeg(u) == 1 and indeg(v) == 1; a unitig is a maximal
chain of links; every k-mer lies in exactly one.  A chain that closes on itself starts at its k-mer of
the smallest row, the link into it cut.  Rows are the BOSS order of real edges: the node (first K - 1
chars) read right to left, then the label.  Unitigs come in ascending row of their first k-mer.

Filters (BOSS::call_unitigs and is_unreliable_unitig of the reference, on the unfiltered graph):
min_tip_size t applies to a unitig of m < t k-mers with first k-mer f and last l -- kept if outdeg(l) >= 2,
else kept if indeg(f) >= 2, else dropped if outdeg(l) == 0, else dropped if indeg(f) == 0, else kept;
min_median_abundance a > 1 drops a unitig when 2 * #{weights < a} > m.
"""
import gzip
import struct

import numpy as np


def count_kmers(K, seqs, canonical=False, bits=8, counts=None):
    """dict k-mer -> count saturated at 2^bits - 1 (bits 0: every count 1)"""
    comp = str.maketrans("ACGT", "TGCA")
    cmax = (1 << bits) - 1 if bits else 1
    cnt = {}
    for idx, seq in enumerate(seqs):
        c = 1 if counts is None else int(counts[idx])
        s = (seq.decode() if isinstance(seq, bytes) else seq).upper().replace("U", "T")
        run = []
        for ch in s + "$":
            if ch in "ACGT":
                run.append(ch)
                continue
            seg = "".join(run)
            run = []
            for i in range(len(seg) - K + 1):
                w = seg[i:i + K]
                cnt[w] = cnt.get(w, 0) + c
                if canonical:
                    r = w.translate(comp)[::-1]
                    cnt[r] = cnt.get(r, 0) + c
    return {w: min(c, cmax) for w, c in cnt.items()}


def boss_order(K, kmers):
    return sorted(kmers, key=lambda s: s[K - 2::-1] + s[K - 1])


def unitigs(K, cnt, min_tip_size=1, min_median_abundance=1, chains=None):
    """-> dict(records=[(sequence, [weights])], dropped_records, dropped_kmers) in output order;
    `chains`: what all_chains(K, cnt) returned, to filter one graph several times"""
    records, dropped_records, dropped_kmers = [], 0, 0
    for p, indeg_f, outdeg_l in all_chains(K, cnt) if chains is None else chains:
        m = len(p)
        keep = True
        if m < min_tip_size:
            if outdeg_l >= 2:
                keep = True
            elif indeg_f >= 2:
                keep = True
            elif outdeg_l == 0:
                keep = False
            elif indeg_f == 0:
                keep = False
        w = [cnt[x] for x in p]
        if min_median_abundance > 1 and 2 * sum(1 for x in w if x < min_median_abundance) > m:
            keep = False
        if keep:
            records.append((p[0] + "".join(x[-1] for x in p[1:]), w))
        else:
            dropped_records += 1
            dropped_kmers += m
    return {"records": records, "dropped_records": dropped_records, "dropped_kmers": dropped_kmers}


def all_chains(K, cnt):
    """every unitig as (its k-mers in path order, indeg(first), outdeg(last)), in output order"""
    outs = {u: [u[1:] + c for c in "ACGT" if u[1:] + c in cnt] for u in cnt}
    ins = {v: [c + v[:-1] for c in "ACGT" if c + v[:-1] in cnt] for v in cnt}
    nxt, linked_into = {}, set()
    for u, o in outs.items():
        if len(o) == 1 and len(ins[o[0]]) == 1:
            nxt[u] = o[0]
            linked_into.add(o[0])
    order = boss_order(K, cnt)
    seen, chains = set(), []

    def walk(h):
        path = [h]
        seen.add(h)
        while path[-1] in nxt and nxt[path[-1]] != h:
            path.append(nxt[path[-1]])
            seen.add(path[-1])
        chains.append(path)

    for h in order:
        if h not in linked_into:
            walk(h)
    for h in order:  # what is left lies on closed chains: the smallest row of each starts it
        if h not in seen:
            walk(h)
    row = {w: i for i, w in enumerate(order)}
    chains.sort(key=lambda p: row[p[0]])
    return [(p, len(ins[p[0]]), len(outs[p[-1]])) for p in chains]


def device_layout(K, records, weighted=True):
    """(seq bytes with one '$' after each record, record_starts u64, counts u32 or None)"""
    seq = b"".join(s.encode() + b"$" for s, _ in records)
    starts = np.zeros(len(records) + 1, np.uint64)
    if records:
        starts[1:] = np.cumsum([len(s) + 1 for s, _ in records])
    counts = np.array([x for _, w in records for x in w], np.uint32) if weighted else None
    return seq, starts, counts


def file_payloads(K, records, weighted=True):
    """what base.fasta.gz and base.kmer_counts.gz decompress to"""
    fasta = b"".join(b">%d\n%s\n" % (i + 1, s.encode()) for i, (s, _) in enumerate(records))
    counts = None
    if weighted:
        counts = struct.pack("<I", K) + np.array([x for _, w in records for x in w], "<u4").tobytes()
    return fasta, counts


def read_gz(path):
    with gzip.open(path, "rb") as f:
        return f.read()
