// unitigs.hpp -- the unitigs of a device chunk with their k-mer counts, as HIP kernels (wave64, gfx950): what
// BOSS::call_unitigs (boss.cpp:2921-3015) over call_paths with split_to_unitigs (boss.cpp:2042-2236) yields,
// filtered as `metagraph clean` filters it (min_tip_size; is_unreliable_unitig, graph_cleaning.cpp:14-32).
//
// A k-mer is a real edge: a row i >= 1 whose node has no '$' and whose label is no '$'.  k-mer u links to v
// when v is the only k-mer u precedes and u the only k-mer preceding v; a unitig is a maximal chain of links.
//
//   W, source flags        -> real[i]                                              (unitig_real_kernel)
//   real, Nav.fwd          -> tgt[i] = last row of i's target node, indeg[tgt] += 1 (unitig_target_kernel)
//   tgt, indeg, last       -> succ / pred links, outdeg(i) and indeg(i) per k-mer   (unitig_link_kernel)
//   pred                   -> (head, distance) by pointer doubling on 64-bit (anc, dist) pairs, one launch
//                             per round, ping-pong buffers, a device flag says whether anything changed
//                             (unitig_rank_init_kernel, unitig_rank_round_kernel)
//   rows unresolved at the cap lie on closed chains: the same doubling carrying the minimum row finds each
//   chain's first k-mer, the link into it is cut and those rows are ranked again
//                             (unitig_cycle_init_kernel, unitig_cycle_round_kernel, unitig_cycle_cut_kernel)
//   -> per unitig: length, last k-mer, weak k-mers; the keep flag      (unitig_stats_kernel, unitig_filter_kernel)
//   -> exclusive scans of the kept lengths and flags (dbgdev::exclusive_scan)
//   -> sequence chars, counts, record starts; each head writes its node by K - 1 Nav.bwd steps
//                             (unitig_emit_kernel, unitig_emit_heads_kernel)
//
// Links are 32-bit (n < 2^32, checked by the host).  Bounds: every thread indexes by a row below n; link and
// navigation targets are clamped to n - 1 or checked against n before they index; output positions are
// checked against the scanned totals that sized the buffers; walks over the rows of one node stop after
// kNodeRows rows, so arrays that are no BOSS table neither leave their buffers nor spin.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbg_device.hpp"

namespace mtg {
namespace unitig {

using dbgdev::kThreads;
using dbgdev::Nav;

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kNodeRows = 8;  // a BOSS node has at most 5 rows

__device__ inline uint64_t pair_of(uint32_t a, uint32_t b) { return (uint64_t)a | ((uint64_t)b << 32); }
__device__ inline uint32_t pair_lo(uint64_t p) { return (uint32_t)p; }
__device__ inline uint32_t pair_hi(uint64_t p) { return (uint32_t)(p >> 32); }

// real[i] = i >= 1 && !source[i] && W[i] % 5 != 0; 16 rows per thread
__global__ __launch_bounds__(kThreads) void unitig_real_kernel(const uint8_t *__restrict__ W,
                                                               const uint8_t *__restrict__ source, uint64_t n,
                                                               uint8_t *__restrict__ real) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (i0 >= n) return;
    uint8_t w[16], f[16];
    const int valid = dbgdev::load16(W, i0, n, w);
    (void)dbgdev::load16(source, i0, n, f);
    uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const bool is = j < valid && i0 + j >= 1 && f[j] == 0 && w[j] < 10 && w[j] % 5 != 0;
        r[j >> 2] |= (uint32_t)is << (8 * (j & 3));
    }
    if (valid == 16 && ((uintptr_t)(real + i0) & 15) == 0) {
        *reinterpret_cast<uint4 *>(real + i0) = make_uint4(r[0], r[1], r[2], r[3]);
    } else {
        for (int j = 0; j < valid; ++j) real[i0 + j] = (uint8_t)(r[j >> 2] >> (8 * (j & 3)));
    }
}

// tgt[i] = the last row of the node edge i leads to; indeg (zeroed) counts the k-mers entering each node there
__global__ __launch_bounds__(kThreads) void unitig_target_kernel(Nav nav, const uint8_t *__restrict__ real,
                                                                 uint32_t *__restrict__ tgt,
                                                                 uint32_t *__restrict__ indeg) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= nav.n) return;
    uint32_t t = kNone;
    if (real[i]) {
        uint64_t j = nav.fwd(i, (uint8_t)(nav.W[i] % 5));
        if (j >= nav.n) j = nav.n - 1;
        t = (uint32_t)j;
        atomicAdd(&indeg[j], 1u);
    }
    tgt[i] = t;
}

// One thread per k-mer i: the k-mers leaving its target node (the real rows of that node) are those it
// precedes; with exactly one, s, and i the only k-mer entering the node, i -> s is a link (a k-mer that links
// to itself is a closed chain of one: the link is cut here).  succ and pred arrive filled with kNone.
__global__ __launch_bounds__(kThreads) void unitig_link_kernel(const uint8_t *__restrict__ real,
                                                               const uint8_t *__restrict__ last, uint64_t n,
                                                               const uint32_t *__restrict__ tgt,
                                                               const uint32_t *__restrict__ indeg,
                                                               uint32_t *__restrict__ succ, uint32_t *__restrict__ pred,
                                                               uint8_t *__restrict__ outdeg_k,
                                                               uint8_t *__restrict__ indeg_k) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || !real[i]) return;
    const uint64_t j = tgt[i];  // < n
    uint32_t out = 0, s = kNone;
    uint64_t r = j;
    for (int step = 0; step < kNodeRows; ++step) {
        if (real[r]) {
            ++out;
            s = (uint32_t)r;
        }
        if (r <= 1 || last[r - 1]) break;
        --r;
    }
    uint64_t e = i;  // the last row of i's own node
    for (int step = 0; step < kNodeRows && !last[e] && e + 1 < n; ++step) ++e;
    const uint32_t in = indeg[e];
    outdeg_k[i] = (uint8_t)(out < 255 ? out : 255);
    indeg_k[i] = (uint8_t)(in < 255 ? in : 255);
    if (out == 1 && indeg[j] == 1 && s != (uint32_t)i) {
        succ[i] = s;
        pred[s] = (uint32_t)i;
    }
}

// state[i] = (anc, dist): (pred, 1), or (kNone, 0) for the first k-mer of a chain and for rows that are no
// k-mer.  `only` (may be null): the rows to set.
__global__ __launch_bounds__(kThreads) void unitig_rank_init_kernel(const uint32_t *__restrict__ pred, uint64_t n,
                                                                    const uint8_t *__restrict__ only,
                                                                    uint64_t *__restrict__ state) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || (only && !only[i])) return;
    const uint32_t p = pred[i];
    state[i] = p == kNone || p >= n ? pair_of(kNone, 0) : pair_of(p, 1);
}

// One doubling round: (anc, dist) -> (anc[anc], dist + dist[anc]) while anc is no first k-mer.  *changed is
// set when any row moved.
__global__ __launch_bounds__(kThreads) void unitig_rank_round_kernel(const uint64_t *__restrict__ in, uint64_t n,
                                                                     uint64_t *__restrict__ out,
                                                                     uint32_t *__restrict__ changed) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool moved = false;
    if (i < n) {
        uint64_t st = in[i];
        const uint32_t a = pair_lo(st);
        if (a != kNone) {
            const uint64_t sa = in[a];  // a < n: a pred or an ancestor of one
            if (pair_lo(sa) != kNone) {
                st = pair_of(pair_lo(sa), pair_hi(st) + pair_hi(sa));
                moved = true;
            }
        }
        out[i] = st;
    }
    if (__ballot(moved) && (threadIdx.x & 63) == 0) *changed = 1;
}

// After the capped rounds a row whose ancestor still has an ancestor lies on a closed chain: cyc[i] = 1 and
// mstate[i] = (pred, min(i, pred)); other rows (kNone, i).  *any is set when a closed chain exists.
__global__ __launch_bounds__(kThreads) void unitig_cycle_init_kernel(const uint64_t *__restrict__ state,
                                                                     const uint32_t *__restrict__ pred, uint64_t n,
                                                                     uint8_t *__restrict__ cyc,
                                                                     uint64_t *__restrict__ mstate,
                                                                     uint32_t *__restrict__ any) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool on = false;
    if (i < n) {
        const uint32_t a = pair_lo(state[i]);
        on = a != kNone && pair_lo(state[a]) != kNone;
        const uint32_t p = on ? pred[i] : kNone;
        on = on && p != kNone && p < n;
        cyc[i] = on;
        mstate[i] = on ? pair_of(p, p < (uint32_t)i ? p : (uint32_t)i) : pair_of(kNone, (uint32_t)i);
    }
    if (__ballot(on) && (threadIdx.x & 63) == 0) *any = 1;
}

// (ptr, min) -> (ptr[ptr], min(min, min[ptr])): after r rounds min covers 2^r predecessors.  When no minimum
// moved in a round, every row holds its chain's smallest row.
__global__ __launch_bounds__(kThreads) void unitig_cycle_round_kernel(const uint64_t *__restrict__ in, uint64_t n,
                                                                      uint64_t *__restrict__ out,
                                                                      uint32_t *__restrict__ changed) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool moved = false;
    if (i < n) {
        uint64_t st = in[i];
        const uint32_t p = pair_lo(st);
        if (p != kNone) {
            const uint64_t sp = in[p];
            const uint32_t m = pair_hi(st), mp = pair_hi(sp);
            moved = mp < m;
            st = pair_of(pair_lo(sp) != kNone ? pair_lo(sp) : p, moved ? mp : m);
        }
        out[i] = st;
    }
    if (__ballot(moved) && (threadIdx.x & 63) == 0) *changed = 1;
}

// the smallest row of a closed chain becomes its first k-mer: the link into it is cut
__global__ __launch_bounds__(kThreads) void unitig_cycle_cut_kernel(const uint8_t *__restrict__ cyc,
                                                                    const uint64_t *__restrict__ mstate, uint64_t n,
                                                                    uint32_t *__restrict__ succ,
                                                                    uint32_t *__restrict__ pred) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || !cyc[i] || pair_hi(mstate[i]) != (uint32_t)i) return;
    const uint32_t q = pred[i];
    pred[i] = kNone;
    if (q < n) succ[q] = kNone;
}

// One thread per k-mer: the last k-mer of a unitig records itself and the length at the unitig's first row;
// k-mers with a weight below `weak_below` are counted there (weak arrives zeroed).
__global__ __launch_bounds__(kThreads) void unitig_stats_kernel(const uint8_t *__restrict__ real,
                                                                const uint64_t *__restrict__ state,
                                                                const uint32_t *__restrict__ succ, uint64_t n,
                                                                const uint32_t *__restrict__ weights,
                                                                uint64_t weak_below, uint32_t *__restrict__ tail,
                                                                uint32_t *__restrict__ len, uint32_t *__restrict__ weak) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || !real[i]) return;
    const uint64_t st = state[i];
    const uint32_t h = pair_lo(st) == kNone ? (uint32_t)i : pair_lo(st);
    if (weights && weak_below > 1 && (uint64_t)weights[i] < weak_below) atomicAdd(&weak[h], 1u);
    if (succ[i] == kNone) {
        tail[h] = (uint32_t)i;
        len[h] = pair_hi(st) + 1;
    }
}

// One thread per row: the keep flag of the unitig that starts here (BOSS::call_unitigs' tip rule, then
// is_unreliable_unitig); klen / kflag = its length / 1 when kept, else 0.  dropped[0..1] += records, k-mers.
__global__ __launch_bounds__(kThreads) void unitig_filter_kernel(const uint8_t *__restrict__ real,
                                                                 const uint64_t *__restrict__ state, uint64_t n,
                                                                 const uint32_t *__restrict__ tail,
                                                                 const uint32_t *__restrict__ len,
                                                                 const uint32_t *__restrict__ weak,
                                                                 const uint8_t *__restrict__ outdeg_k,
                                                                 const uint8_t *__restrict__ indeg_k,
                                                                 uint64_t min_tip, int filter_weak,
                                                                 uint32_t *__restrict__ klen, uint32_t *__restrict__ kflag,
                                                                 unsigned long long *__restrict__ dropped) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint64_t drop_rec = 0, drop_kmers = 0;
    if (i < n) {
        uint32_t m = 0;
        bool keep = false;
        if (real[i] && pair_lo(state[i]) == kNone) {
            m = len[i];
            uint32_t l = tail[i];
            if (l >= n) l = (uint32_t)i;
            keep = true;
            if ((uint64_t)m < min_tip) {
                const uint32_t od = outdeg_k[l], id = indeg_k[i];
                if (od >= 2) keep = true;
                else if (id >= 2) keep = true;
                else if (od == 0) keep = false;
                else if (id == 0) keep = false;
            }
            if (filter_weak && 2 * (uint64_t)weak[i] > m) keep = false;
            if (!keep) {
                drop_rec = 1;
                drop_kmers = m;
            }
        }
        klen[i] = keep ? m : 0;
        kflag[i] = keep ? 1 : 0;
    }
    drop_rec = dbgdev::wave_sum(drop_rec);
    drop_kmers = dbgdev::wave_sum(drop_kmers);
    if ((threadIdx.x & 63) == 0 && drop_rec) {
        atomicAdd(&dropped[0], (unsigned long long)drop_rec);
        atomicAdd(&dropped[1], (unsigned long long)drop_kmers);
    }
}

struct EmitOut {
    uint8_t *seq;
    uint64_t seq_len;
    uint64_t *record_starts;
    uint64_t n_records;
    uint32_t *counts;  // or null
    uint64_t n_kmers;
    uint64_t K;  // chars of a k-mer
};

// One thread per k-mer of a kept unitig: its label at seq_off + (K - 1) + d, its weight at cnt_off + d, where
// cnt_off = the scan of kept lengths at the unitig's first row and seq_off = cnt_off + K * (record index).
__global__ __launch_bounds__(kThreads) void unitig_emit_kernel(const uint8_t *__restrict__ W,
                                                               const uint8_t *__restrict__ real,
                                                               const uint64_t *__restrict__ state, uint64_t n,
                                                               const uint32_t *__restrict__ kflag,
                                                               const uint64_t *__restrict__ cnt_off,
                                                               const uint64_t *__restrict__ rec_idx,
                                                               const uint32_t *__restrict__ weights, EmitOut o) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i == 0) o.record_starts[o.n_records] = o.seq_len;
    if (i >= n || !real[i]) return;
    const uint64_t st = state[i];
    const uint32_t h = pair_lo(st) == kNone ? (uint32_t)i : pair_lo(st);
    if (!kflag[h]) return;
    const uint64_t d = pair_hi(st), co = cnt_off[h] + d;
    const uint64_t so = cnt_off[h] + rec_idx[h] * o.K + (o.K - 1) + d;
    if (so < o.seq_len) o.seq[so] = "$ACGT"[W[i] % 5];
    if (o.counts && co < o.n_kmers) o.counts[co] = weights[i];
}

// One thread per kept unitig (at its first row): the record start, the separator after the record, and the
// first k-mer's node, last char first, by K - 1 steps backwards.
__global__ __launch_bounds__(kThreads) void unitig_emit_heads_kernel(Nav nav, const uint32_t *__restrict__ kflag,
                                                                     const uint32_t *__restrict__ klen,
                                                                     const uint64_t *__restrict__ cnt_off,
                                                                     const uint64_t *__restrict__ rec_idx, EmitOut o) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= nav.n || !kflag[i]) return;
    const uint64_t rec = rec_idx[i], so = cnt_off[i] + rec * o.K, end = so + (o.K - 1) + klen[i];
    if (rec < o.n_records) o.record_starts[rec] = so;
    if (end < o.seq_len) o.seq[end] = '$';
    uint64_t row = i;
    for (uint64_t t = 1; t < o.K; ++t) {
        const uint8_t c = nav.node_last_char(row);
        const uint64_t at = so + (o.K - 1) - t;
        if (at < o.seq_len) o.seq[at] = "$ACGT"[c];
        if (t + 1 < o.K) row = nav.bwd(row);
    }
}

}  // namespace unitig
}  // namespace mtg
