// kmer_counts.hpp -- contigs with per-k-mer counts (X.fasta.gz + X.kmer_counts.gz) as counted reads.
//
// `metagraph clean` and `transform --to-fasta` write, next to the contigs, a counts file: a u32 k
// followed by one u32 per k-mer window, record after record.  `build --count-kmers` reads the pair back
// with read_extended_fasta_file_critical (seq_io/sequence_io.cpp:407-467) and parse_sequences cuts every
// record into its runs of equal counts, one add_sequence(run + k - 1 chars, count) per run
// (cli/parse_sequences.hpp:120-138).  The runs of a record partition its windows, and the extractor
// gives a window the count of the last read start at or before it (read_of, device_common.hpp), so a
// run is just a (start, count) pair over the unsegmented sequence: no sequence byte moves.
//
// Input, on the device: the record starts of the split FASTA (record r = [rs[r], rs[r + 1] - 1), one
// separator byte after every record; rs has n_rec + 1 entries), the counts payload, the DBG k.
//   windows -- per record L_r - k + 1 (a record shorter than k, or starts that do not ascend, raise the
//              error flag), scanned by scan_counts into woff: record r's counts are counts[woff[r] ..).
//   runs    -- count and write passes over tiles of KC_TILE sequence positions (the count / scan /
//              write shape of fasta_split_kernel): position p is window i = p - rs[r] of its record when
//              i < L_r - k + 1 and opens a run when i == 0 or its count differs from the window before.
//              The tile's counts (a contiguous span of at most KC_TILE + 1 entries) come in with 16-byte
//              loads into LDS; the write pass compacts the runs in LDS and stores them contiguously at
//              the tile's scanned offset.  No global atomics but the error flag.
// Invalid characters inside a record change nothing here: the counts file has an entry for every
// position, and the extractor drops those windows.  Counts are passed on as they are (the extractor
// saturates them at the count width).  Included by boss_pipeline.hip only.
#pragma once

#include "ctx.hpp"
#include "device_common.hpp"
#include "sort_unique.hpp"

namespace mtg {

constexpr int KC_BLOCK = 256;
constexpr int KC_PER = 8;                     // sequence positions per thread
constexpr int KC_TILE = KC_BLOCK * KC_PER;    // sequence positions per tile
constexpr int KC_SPAN = KC_TILE + 8;          // a tile's counts: its windows, the one before, 16-byte alignment

// the caller's input is no counted FASTA: the entry points return MTG_ERR_ARGUMENT
struct KmerCountsError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// wcnt[r] = windows of record r; *bad |= 1: a record shorter than k (or starts that do not ascend),
// |= 2: a record of 2^32 windows or more
__global__ __launch_bounds__(256) void kc_windows_kernel(const uint64_t *__restrict__ rs, uint64_t n_rec, uint32_t k,
                                                         uint32_t *__restrict__ wcnt, uint32_t *__restrict__ bad) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += gs) {
        const uint64_t a = rs[r], b = rs[r + 1];
        uint32_t w = 0, e = 0;
        if (b <= a || b - 1 - a < k) {
            e = 1;
        } else {
            const uint64_t nw = b - 1 - a - k + 1;
            if (nw > 0xFFFFFFFFull) e = 2;
            else w = (uint32_t)nw;
        }
        wcnt[r] = w;
        if (e) atomicOr(bad, e);
    }
}

// the last r in [lo, hi) with rs[r] <= p (rs[lo] <= p)
__device__ __forceinline__ uint64_t kc_record_of(const uint64_t *__restrict__ rs, uint64_t lo, uint64_t hi, uint64_t p) {
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (rs[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

/*
 * count (WRITE = false: tcnt[t] = runs opened in tile t) and write (the runs at toff[t] of read_starts /
 * read_counts, in position order) passes over the same tiles.  Tile t holds positions rs[0] + t KC_TILE ..;
 * the windows pass has checked that every record has a window and that woff[n_rec] == n_counts, so the
 * count index woff[r] + min(i, windows of r) ascends by at most one per position.
 */
template <bool WRITE>
__global__ __launch_bounds__(KC_BLOCK) void kc_runs_kernel(const uint64_t *__restrict__ rs, uint64_t n_rec,
                                                           const uint64_t *__restrict__ woff,
                                                           const uint32_t *__restrict__ counts, uint64_t n_counts,
                                                           uint32_t k, uint32_t *__restrict__ tcnt,
                                                           const uint64_t *__restrict__ toff,
                                                           uint64_t *__restrict__ read_starts,
                                                           uint32_t *__restrict__ read_counts, uint64_t out_base) {
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[KC_SPAN];
    __shared__ uint32_t s_scan[KC_BLOCK / 64 + 1];
    __shared__ uint64_t s_edge[4];  // the records and count indices of the tile's first and last position
    __shared__ uint32_t s_off[WRITE ? KC_TILE : 1];
    __shared__ uint32_t s_val[WRITE ? KC_TILE : 1];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x;
    const uint64_t p_end = rs[n_rec];  // one past the last record's separator
    const uint64_t tile_p = rs[0] + t * KC_TILE;
    if (tile_p >= p_end) {  // (the host sizes the grid by the span: no such tile)
        if (!WRITE && tid == 0) tcnt[t] = 0;
        return;
    }
    const uint64_t tile_last = min(tile_p + KC_TILE, p_end) - 1;
    auto cidx = [&](uint64_t r, uint64_t p) {  // the count index of position p in record r
        const uint64_t a = rs[r], i = p - a, nw = rs[r + 1] - a - k;
        return woff[r] + min(i, nw);
    };
    if (tid < 2) {
        const uint64_t p = tid ? tile_last : tile_p;
        const uint64_t r = kc_record_of(rs, 0, n_rec, p);
        s_edge[tid] = r;
        s_edge[2 + tid] = cidx(r, p);
    }
    __syncthreads();
    const uint64_t r_lo = s_edge[0], r_hi = s_edge[1];
    // the tile's counts -> LDS: [c_lo, c_hi) with 16-byte loads from the aligned index below c_lo
    const uint64_t c_lo = s_edge[2] ? s_edge[2] - 1 : 0, c_hi = min(s_edge[3] + 1, n_counts);
    const int64_t mis = (int64_t)(((uintptr_t)counts >> 2) & 3);
    const int64_t c_al = (int64_t)c_lo - (int64_t)(((int64_t)c_lo + mis) & 3);
    for (int64_t v = tid; c_al + 4 * v < (int64_t)c_hi && 4 * v + 3 < KC_SPAN; v += KC_BLOCK) {
        const int64_t i = c_al + 4 * v;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (i >= 0 && (uint64_t)i + 4 <= n_counts) {
            q = *reinterpret_cast<const uint4 *>(counts + i);
        } else {
            if (i >= 0 && (uint64_t)i < n_counts) q.x = counts[i];
            if (i + 1 >= 0 && (uint64_t)(i + 1) < n_counts) q.y = counts[i + 1];
            if (i + 2 >= 0 && (uint64_t)(i + 2) < n_counts) q.z = counts[i + 2];
            if (i + 3 >= 0 && (uint64_t)(i + 3) < n_counts) q.w = counts[i + 3];
        }
        *reinterpret_cast<uint4 *>(&s_cnt[4 * v]) = q;
    }
    __syncthreads();
    auto count_at = [&](uint64_t ci) { return s_cnt[min((uint64_t)(KC_SPAN - 1), (uint64_t)((int64_t)ci - c_al))]; };
    const uint64_t p0 = tile_p + (uint64_t)tid * KC_PER;
    uint32_t opens = 0, mask = 0;
    uint32_t val[KC_PER];
#pragma unroll
    for (int j = 0; j < KC_PER; ++j) val[j] = 0;
    if (p0 <= tile_last) {
        uint64_t r = kc_record_of(rs, r_lo, r_hi + 1, p0);
        uint64_t a = rs[r], b = rs[r + 1], w = woff[r];
#pragma unroll
        for (int j = 0; j < KC_PER; ++j) {
            const uint64_t p = p0 + j;
            if (p > tile_last) break;
            while (p >= b && r + 1 < n_rec) {
                ++r;
                a = b;
                b = rs[r + 1];
                w = woff[r];
            }
            const uint64_t i = p - a, nw = b - a - k;
            if (i < nw) {
                const uint32_t cv = count_at(w + i);
                if (i == 0 || cv != count_at(w + i - 1)) {
                    ++opens;
                    mask |= 1u << j;
                    val[j] = cv;
                }
            }
        }
    }
    uint32_t total;
    const uint32_t off = block_exclusive_sum<KC_BLOCK>(opens, s_scan, &total);
    if constexpr (!WRITE) {
        if (tid == 0) tcnt[t] = total;
    } else {
        uint32_t o = off;
#pragma unroll
        for (int j = 0; j < KC_PER; ++j) {
            if ((mask >> j) & 1u) {
                s_off[o] = tid * KC_PER + j;
                s_val[o] = val[j];
                ++o;
            }
        }
        __syncthreads();
        const uint64_t ob = out_base + toff[t];
        for (uint32_t q = tid; q < total; q += KC_BLOCK) {
            read_starts[ob + q] = tile_p + s_off[q];
            read_counts[ob + q] = s_val[q];
        }
    }
}

// One counted file (or caller-held arrays) on the device, between its two host syncs: plan() checks the
// records against the counts and returns the runs; write() stores them.
struct KmerCountRuns {
    const uint64_t *rs = nullptr;
    uint64_t n_rec = 0;
    const uint32_t *counts = nullptr;
    uint64_t n_counts = 0;
    uint32_t k = 0;
    uint64_t tiles = 0, n_runs = 0;
    const uint64_t *woff = nullptr, *toff = nullptr;

    // seq_span = rs[n_rec] - rs[0] (the caller knows it, or reads it back)
    uint64_t plan(Ctx &c, uint64_t seq_span) {
        n_runs = 0;
        if (!n_rec) {
            if (n_counts) throw KmerCountsError("ERROR: There are features left in extension unread");
            return 0;
        }
        hipStream_t s = c.stream;
        uint32_t *wcnt = (uint32_t *)c.ws.get(Workspace::KC_WCNT, n_rec * 4);
        uint64_t *wo = (uint64_t *)c.ws.get(Workspace::KC_WOFF, (n_rec + 1) * 8);
        HIP_CHECK(hipMemsetAsync(&c.small->kc_bad, 0, 4, s));
        HIP_CHECK(hipMemsetAsync(&c.small->error, 0, 4, s));  // the scans' look-back word: checked below
        kc_windows_kernel<<<dim3((unsigned)std::min<uint64_t>(ceil_div(n_rec, 256), 4096)), dim3(256), 0, s>>>(
            rs, n_rec, k, wcnt, &c.small->kc_bad);
        HIP_CHECK(hipGetLastError());
        scan_counts(c, wcnt, n_rec, wo);
        uint32_t bad = 0;
        HIP_CHECK(hipMemcpyAsync(&bad, &c.small->kc_bad, 4, hipMemcpyDeviceToHost, s));
        const uint64_t windows = read_u64(c, (const unsigned long long *)(wo + n_rec));
        if (bad & 1u)
            throw KmerCountsError("ERROR: Bad fasta file. Found sequence shorter than k-mer length " + std::to_string(k));
        if (bad) throw KmerCountsError("ERROR: a sequence with more than 2^32 - 1 k-mer counts is not supported");
        if (windows > n_counts) throw KmerCountsError("ERROR: Cannot read k-mer features");
        if (windows < n_counts) throw KmerCountsError("ERROR: There are features left in extension unread");
        woff = wo;
        tiles = ceil_div(seq_span, KC_TILE);
        if (tiles > 0x7FFFFFFFull) throw KmerCountsError("ERROR: the counted sequences are too long for one file");
        uint32_t *tcnt = (uint32_t *)c.ws.get(Workspace::KC_TCNT, (tiles + 1) * 4);
        uint64_t *to = (uint64_t *)c.ws.get(Workspace::KC_TOFF, (tiles + 1) * 8);
        kc_runs_kernel<false><<<dim3((unsigned)tiles), dim3(KC_BLOCK), 0, s>>>(rs, n_rec, woff, counts, n_counts, k, tcnt,
                                                                             nullptr, nullptr, nullptr, 0);
        HIP_CHECK(hipGetLastError());
        n_runs = scan_counts_total(c, tcnt, tiles, to);
        check_error_word(c);
        toff = to;
        return n_runs;
    }

    // the runs to read_starts / read_counts [out_base, out_base + n_runs)
    void write(Ctx &c, uint64_t *read_starts, uint32_t *read_counts, uint64_t out_base) const {
        if (!n_runs) return;
        kc_runs_kernel<true><<<dim3((unsigned)tiles), dim3(KC_BLOCK), 0, c.stream>>>(
            rs, n_rec, woff, counts, n_counts, k, nullptr, toff, read_starts, read_counts, out_base);
        HIP_CHECK(hipGetLastError());
    }
};

}  // namespace mtg
