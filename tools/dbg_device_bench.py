#!/usr/bin/env python3
"""From a device chunk to the graph files, two ways, at the bench's configs[1] workload.

(a) the host writer: W / last / weights copied to the host, `last` packed, mtg_boss_write_dbg;
(b) mtg_boss_write_dbg_device on the chunk where it lies, with its device / copy / host split.
Each path runs once after one warm-up, both write --mask-dummy files with the default suffix index,
and the two file sets are compared byte for byte.  Prints one JSON line and writes it to --out.
Set MTG_TRACE=1 to get the host remainder of (b) by container on stderr.

--prune times `concatenate --clear-dummy` instead: the suffix chunks (--suffix-len) of a FASTA file are
built on the GPU, concatenated, and pruned and written (c) by the host writer (prune=True) from the
concatenated host chunk and (d) by mtg_boss_write_dbg_device_pruned from the same rows uploaded, in
basic and canonical mode, with the same comparison.

--unitigs times mtg_boss_unitigs_device on the workload's counted chunk (events on the call's stream), reports
its ranking rounds, records and k-mers, and times the rebuild from its output (profiles/unitigs_bench.json)."""
import argparse
import ctypes
import filecmp
import importlib
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def prune_main(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seq_io  # tests/seq_io.py: the FASTA reader of the tests
    boss = importlib.import_module("projects2014-metagenome_amd.boss")
    if boss.device_count() < 1:
        sys.exit("dbg_device_bench: no GPU (a measurement does not fall back)")
    seqs = seq_io.read_sequences(args.fasta)
    kb = args.k - 1
    L = boss.lib()
    parent = args.dir or ("/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    out_dir = tempfile.mkdtemp(prefix="mtg_dbg_bench_", dir=parent)
    modes, ok = {}, True
    try:
        for name, both in (("basic", False), ("canonical", True)):
            chunks = []
            for suf in boss.generate_suffixes(args.suffix_len):
                c = boss.IBOSSChunkConstructor.initialize(kb, both_strands=both, filter_suffix=suf)
                c.add_sequences(seqs)
                chunks.append(c.build_chunk())
            cat = boss.concatenate(chunks)
            n = len(cat.W)
            writer = boss.IBOSSChunkConstructor.initialize(kb, both_strands=both)
            dc = boss._DeviceChunk(k=kb, n=n)
            ptrs = []
            for field, arr in (("W", np.ascontiguousarray(cat.W, np.uint8)), ("last", np.ascontiguousarray(cat.last, np.uint8))):
                d = L.mtg_device_alloc(0, n)
                assert d and L.mtg_memcpy_h2d(d, arr.ctypes.data, n) == 0
                ptrs.append(d)
                setattr(dc, field, d)
            dc.F = (ctypes.c_uint64 * 5)(*[int(f) for f in cat.F])
            host_chunk = boss.Chunk(kb, cat.W, None, cat.F, last_words=boss.pack_last(cat.last))

            def host_path(base):
                t0 = time.perf_counter()
                nv = host_chunk.write_dbg(base, canonical=both, mask_dummy=True, prune=True)
                return nv, {"write_dbg_s": time.perf_counter() - t0}

            def device_path(base):
                t0 = time.perf_counter()
                nv = writer.write_dbg_device(dc, base, canonical=both, prune=True)
                split = dict(writer.last_dbg_timings)
                split["total_s"] = time.perf_counter() - t0
                split["n_erased"] = int(writer.last_dbg_erased)
                return nv, split

            host_path(os.path.join(out_dir, "warm_h"))
            device_path(os.path.join(out_dir, "warm_d"))
            nv_h, host = host_path(os.path.join(out_dir, "h"))
            nv_d, dev = device_path(os.path.join(out_dir, "d"))
            same = not os.path.exists(os.path.join(out_dir, "d.dbg.weights"))
            for ext in (".dbg", ".edgemask"):
                same = same and filecmp.cmp(os.path.join(out_dir, "h" + ext), os.path.join(out_dir, "d" + ext), shallow=False)
            for d in ptrs:
                L.mtg_device_free(d)
            ok = ok and same and nv_h == nv_d
            modes[name] = {"rows": n, "host_writer": host, "device_writer": dev,
                           "ratio_host_over_device": host["write_dbg_s"] / dev["total_s"],
                           "n_valid": int(nv_d), "n_valid_equal": bool(nv_h == nv_d), "bytes_equal": bool(same)}
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    res = {"workload": "%s: suffix chunks of length %d, DBG k = %d, concatenated, pruned and written"
                       % (os.path.basename(args.fasta), args.suffix_len, args.k),
           "directory": parent,
           "protocol": "each path once after one warm-up; wall clock around calls that end synchronised; the "
                       "host time excludes the copy of the chunk to the host, the device time the upload",
           "modes": modes}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


def unitigs_main(args):
    """build -> unitigs with counts -> rebuild, all on the device: one sample after one warm-up"""
    import torch
    import bench
    boss = importlib.import_module("projects2014-metagenome_amd.boss")
    if not torch.cuda.is_available():
        sys.exit("dbg_device_bench: no GPU (a measurement does not fall back)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    seq = bench.make_reads_device(torch, args.reads, args.read_len, 1000, "genome", 10.0, device)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    kb, width = args.k - 1, args.count_width or 8
    ctor = boss.IBOSSChunkConstructor.initialize(kb, both_strands=True, bits_per_count=width)
    dc = ctor.build_device(seq.data_ptr(), seq.numel())
    build_ms = ctor.timings().total_ms
    stream = torch.cuda.Stream(device)
    rebuild = boss.IBOSSChunkConstructor.initialize(kb, both_strands=False, bits_per_count=width)

    def once():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(stream)
        u = ctor.unitigs_device(dc, stream=stream.cuda_stream)
        ev[1].record(stream)
        ev[1].synchronize()
        t0 = time.perf_counter()
        runs = rebuild.kmer_counts_to_reads(*u.counts_args())
        dc2 = rebuild.build_device(*u.build_args(runs))
        wall = time.perf_counter() - t0
        return {"unitigs_device_ms": ev[0].elapsed_time(ev[1]), "ranking_rounds": int(ctor.unitigs_last_rounds()),
                "records": int(u.n_records), "kmers": int(u.n_kmers), "seq_bytes": int(u.seq_len),
                "rebuild_wall_s": wall, "rebuild_device_ms": rebuild.timings().total_ms,
                "rebuilt_rows": int(dc2.n), "rebuilt_real": int(dc2.n_real)}

    once()
    sample = once()
    ok = sample["kmers"] == int(dc.n_real) == sample["rebuilt_real"]
    res = {"workload": "configs[1] generator: %d reads of %d bp, DBG k = %d, canonical, count width %d"
                       % (args.reads, args.read_len, args.k, width),
           "gpu": torch.cuda.get_device_name(0), "rows": int(dc.n), "real_edges": int(dc.n_real),
           "build_device_ms": build_ms,
           "protocol": "one sample after one warm-up; unitigs_device_ms between events on the call's stream (the "
                       "call's host synchronisations included); the rebuild is a basic-mode counted build of the "
                       "unitigs of both strands",
           "unitigs": sample, "kmers_equal": bool(ok)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31, help="DBG k (BOSS k = k - 1)")
    ap.add_argument("--count-width", type=int, default=0)
    ap.add_argument("--dir", default=None, help="where the files go (default: a fresh directory on /dev/shm or $TMPDIR)")
    ap.add_argument("--out", default=None, help="default: profiles/dbg_device_bench.json, dbg_prune_bench.json with --prune")
    ap.add_argument("--prune", action="store_true", help="time the pruned writers on concatenated suffix chunks")
    ap.add_argument("--fasta", default=os.path.join(ROOT, "tests", "golden", "transcripts_1000.fa"))
    ap.add_argument("--suffix-len", type=int, default=1)
    ap.add_argument("--unitigs", action="store_true",
                    help="time mtg_boss_unitigs_device on the counted chunk and the rebuild from its output")
    args = ap.parse_args()
    if args.out is None:
        name = "dbg_prune_bench.json" if args.prune else "unitigs_bench.json" if args.unitigs else "dbg_device_bench.json"
        args.out = os.path.join(ROOT, "profiles", name)
    if args.prune:
        return prune_main(args)
    if args.unitigs:
        return unitigs_main(args)

    import torch
    import bench
    boss = importlib.import_module("projects2014-metagenome_amd.boss")
    if not torch.cuda.is_available():
        sys.exit("dbg_device_bench: no GPU (a measurement does not fall back)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    seq = bench.make_reads_device(torch, args.reads, args.read_len, 1000, "genome", 10.0, device)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    kb = args.k - 1
    ctor = boss.IBOSSChunkConstructor.initialize(kb, both_strands=True, bits_per_count=args.count_width)
    dc = ctor.build_device(seq.data_ptr(), seq.numel())
    build_ms = ctor.timings().total_ms
    n = int(dc.n)

    parent = args.dir or ("/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    out_dir = tempfile.mkdtemp(prefix="mtg_dbg_bench_", dir=parent)
    L = boss.lib()

    def host_path(base):
        t0 = time.perf_counter()
        W = np.empty(n, np.uint8)
        last = np.empty(n, np.uint8)
        assert L.mtg_memcpy_d2h(W.ctypes.data, dc.W, n) == 0
        assert L.mtg_memcpy_d2h(last.ctypes.data, dc.last, n) == 0
        weights = None
        if args.count_width:
            weights = np.empty(n, np.uint32)
            assert L.mtg_memcpy_d2h(weights.ctypes.data, dc.weights, 4 * n) == 0
        t1 = time.perf_counter()
        ch = boss.Chunk(kb, W, None, np.array(list(dc.F), np.uint64), weights, bits_per_count=args.count_width,
                        last_words=boss.pack_last(last))
        t2 = time.perf_counter()
        nv = ch.write_dbg(base, canonical=True, mask_dummy=True)
        t3 = time.perf_counter()
        return nv, {"d2h_s": t1 - t0, "pack_last_s": t2 - t1, "write_dbg_s": t3 - t2, "total_s": t3 - t0,
                    "d2h_bytes": n * (2 + (4 if args.count_width else 0))}

    def device_path(base):
        t0 = time.perf_counter()
        nv = ctor.write_dbg_device(dc, base, canonical=True, mask_dummy=True)
        t1 = time.perf_counter()
        split = dict(ctor.last_dbg_timings)
        split["total_s"] = t1 - t0
        return nv, split

    try:
        host_path(os.path.join(out_dir, "warm_h"))
        device_path(os.path.join(out_dir, "warm_d"))
        nv_h, host = host_path(os.path.join(out_dir, "h"))
        nv_d, dev = device_path(os.path.join(out_dir, "d"))
        same, sizes = True, {}
        for ext in (".dbg", ".edgemask", ".dbg.weights"):
            h, d = os.path.join(out_dir, "h" + ext), os.path.join(out_dir, "d" + ext)
            if os.path.exists(h) != os.path.exists(d):
                same = False
            elif os.path.exists(h):
                sizes[ext] = os.path.getsize(h)
                same = same and filecmp.cmp(h, d, shallow=False)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    res = {
        "workload": "configs[1] generator: %d reads of %d bp, DBG k = %d, canonical, count width %d"
                    % (args.reads, args.read_len, args.k, args.count_width),
        "gpu": torch.cuda.get_device_name(0),
        "rows": n, "build_device_ms": build_ms, "directory": parent, "file_bytes": sizes,
        "protocol": "each path once after one warm-up; wall clock around calls that end synchronised",
        "host_writer": host, "device_writer": dev,
        "ratio_host_over_device": host["total_s"] / dev["total_s"],
        "n_valid": int(nv_d), "n_valid_equal": bool(nv_h == nv_d), "bytes_equal": bool(same),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same and nv_h == nv_d else 1


if __name__ == "__main__":
    sys.exit(main())
