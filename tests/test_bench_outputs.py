"""bench.py --dump-outputs: the sample of rows it stores, the files it writes (against host arrays
standing in for the device chunk, and on the GPU against the oracle), and what a plain run leaves
to --full."""
import ctypes
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import bench

_BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")


def test_dump_sample_rows_fixed_and_bounded():
    assert np.array_equal(bench.dump_sample_rows(1000), np.arange(1000))
    n = bench.DUMP_SAMPLE_ROWS * 3 + 17
    a, b = bench.dump_sample_rows(n), bench.dump_sample_rows(n)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_SAMPLE_ROWS
    assert np.all(np.diff(a) >= 0) and a[0] >= 0 and a[-1] < n
    # W, last, weights as float32 at these rows, the rows themselves as float64
    assert bench.DUMP_SAMPLE_ROWS * (3 * 4 + 8) + 8 * (5 + 3 + 256 + 2) <= 64_000_000


class _HostLib:
    """mtg_memcpy_d2h over host memory: the "device" pointers of the fake chunk are numpy buffers."""

    @staticmethod
    def mtg_memcpy_d2h(dst, src, nbytes):
        ctypes.memmove(dst, src, nbytes)
        return 0


@pytest.mark.parametrize("weights", [False, True])
def test_dump_outputs_files(tmp_path, monkeypatch, weights):
    # more rows than the sample and than one block (a ragged last block): every row is summarised,
    # the stored rows are the seeded sample
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ROWS", 1000)
    rng = np.random.default_rng(5)
    n = 10_007
    W = rng.integers(0, 10, size=n, dtype=np.uint8)
    last = rng.integers(0, 2, size=n, dtype=np.uint8)
    wt = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    dc = types.SimpleNamespace(n=n, W=W.ctypes.data, last=last.ctypes.data,
                               weights=wt.ctypes.data if weights else None,
                               F=[0, 1, 20, 300, 4000], n_real=9000, n_dummy=1006)
    fake = types.SimpleNamespace(lib=lambda: _HostLib)
    out = str(tmp_path / "dump")
    bench.dump_outputs(out, fake, dc, weights, block=4096)
    rows = bench.dump_sample_rows(n, 1000)
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert set(got) == {"rows", "W", "last", "F", "summary"} | ({"weights"} if weights else set())
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["rows"], rows)
    assert np.array_equal(got["W"], W[rows]) and np.array_equal(got["last"], last[rows])
    assert np.array_equal(got["F"], [0, 1, 20, 300, 4000])
    s = got["summary"]
    assert list(s[:3]) == [n, 9000, 1006]
    assert np.array_equal(s[3:259], np.bincount(W, minlength=256))
    assert s[259] == np.count_nonzero(last)
    if weights:
        assert np.array_equal(got["weights"], wt[rows].astype(np.float32))
        assert s[260] == int(wt.sum(dtype=np.uint64))
    else:
        assert s[260] == 0


def test_bench_rejects_zero_steps():
    out = subprocess.run([sys.executable, _BENCH, "--gpus", "1", "--steps", "0"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode != 0 and "--steps" in out.stderr


@pytest.mark.gpu
def test_plain_bench_dumps_the_oracle_chunk(tmp_path):
    # a plain run on 20 k reads: 3 timed steps, the result line without the --full legs, and the
    # dumped chunk (all rows: fewer than the sample) equal to the oracle's on the same reads
    import torch
    import oracle_ctypes as O
    n_reads, L, k = 20_000, 150, 31
    out = str(tmp_path / "dump")
    run = subprocess.run([sys.executable, _BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--reads", str(n_reads), "--dump-outputs", out],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n_reads * (L - k + 1) / (line["ms_per_step"] * 1e-3))
    for moved in ("cpu_baseline", "parity", "host_path", "hot_path_host_arrays", "fasta_path"):
        assert moved not in line
    assert line["roofline"]["peak_measured"] is None

    seq = bench.make_reads_device(torch, n_reads, L, 1000, "genome", 10.0, torch.device("cuda", 0))
    want = O.build_chunk_packed(k - 1, seq.cpu().numpy(),
                                np.arange(n_reads + 1, dtype=np.uint64) * (L + 1), canonical=True,
                                bits_per_count=0)
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert set(got) == {"rows", "W", "last", "F", "summary"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    n = len(want.W)
    assert n < bench.DUMP_SAMPLE_ROWS and np.array_equal(got["rows"], np.arange(n))
    assert np.array_equal(got["W"], want.W) and np.array_equal(got["last"], want.last)
    assert np.array_equal(got["F"], want.F)
    assert got["summary"][0] == n and got["summary"][0] == line["counts"]["n_rows"]
    assert np.array_equal(got["summary"][3:259], np.bincount(want.W, minlength=256))
