// dbg_prune.hpp -- `concatenate --clear-dummy` on a device chunk: dbgio::prune_dummy_edges (dbg_io.hpp)
// as HIP kernels (wave64, gfx950), bit for bit.
//
//   W -> single[i], "edge i is the only edge into its target": a suffix scan over the rows
//   roots -> the source-dummy tree level by level, every level kept (edge row, slot of its parent)
//   deepest level -> roots: an inner edge is needed when a child is; redundant = visited && !needed
//   erase_edges: a compaction over all rows; the minus labels whose first occurrence was erased lose
//         their minus (a prefix scan over the rows), `last` moves to the previous kept row, F counts
//         the kept rows
//
// Both scans carry the same small state across rows: per label class c = W % 5 what the last row of the
// class seen so far was (2 bits each).  A later row of the class overwrites the field, so the operator
// is associative and the scan runs like the count scan: a state per tile, one block scanning the tile
// states, every tile rescanned from its carried state.  An erased run of any length leaves the fields of
// the other classes alone, so the carried state crosses any number of tiles.
//
// Bounds: the level pool holds n entries and the host checks the sum of the levels against n before a
// level is written; rows read through a level entry are rows the walk produced below n (clamped again
// where they come from navigation); the compaction writes at the scanned count of kept rows, below n.
#pragma once

#include "dbg_device.hpp"

namespace mtg {
namespace dbgdev {

// ------------------------------------------------------------------------ the class-state scan

// five 2-bit fields, class c at bits 2c: 0 = no row of the class yet, else the kind of the last one
__device__ inline uint32_t state_combine(uint32_t earlier, uint32_t later) {
    const uint32_t m = (later | (later >> 1)) & 0x155u;
    return (earlier & ~(m * 3u)) | later;
}

__device__ inline uint32_t wave_incl_scan_state(uint32_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x = state_combine(y, x);
    }
    return x;
}

// exclusive scan of one state per thread over the 256-thread block; *total = all of them combined
__device__ inline uint32_t block_excl_scan_state(uint32_t x, uint32_t *total, uint32_t *lds /* 4 words */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan_state(x);
    uint32_t excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0;
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const uint32_t s = lds[w];
        if (w < wave) base = state_combine(base, s);
        tot = state_combine(tot, s);
    }
    __syncthreads();
    *total = tot;
    return state_combine(base, excl);
}

// The two scans.  kSingle runs over the rows backwards (position p is row n - 1 - p) and records per
// class whether the last row seen was plain (1) or a minus label (2).  kErase runs forwards and records
// per class whether an erased plain row (2) or a kept row (1) came last.
enum { kSingle = 0, kErase = 1 };

template <int MODE>
__device__ inline uint32_t row_state(uint8_t w, bool erased) {
    const uint32_t c = w % 5;
    if (MODE == kSingle) return c ? (w > 5 ? 2u : 1u) << (2 * c) : 0u;
    if (erased) return w < 5 ? 2u << (2 * w) : 0u;
    return 1u << (2 * c);
}

// 16 positions of one thread from p0: the rows' labels and erase flags (0 past n; callers test p0 + j < n)
template <int MODE>
__device__ inline void load_rows(const uint8_t *__restrict__ W, const uint8_t *__restrict__ erase, uint64_t n,
                                 uint64_t p0, uint8_t w[16], uint8_t er[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint64_t p = p0 + j;
        const bool in = p < n;
        const uint64_t i = in ? (MODE == kSingle ? n - 1 - p : p) : 0;
        w[j] = in ? W[i] : (uint8_t)0;
        er[j] = (MODE == kErase && in) ? erase[i] : (uint8_t)0;
    }
}

// tstate[tile] = the tile's rows combined; tcount[tile] = its kept rows (kErase)
template <int MODE>
__global__ __launch_bounds__(kThreads) void state_tile_kernel(const uint8_t *__restrict__ W,
                                                              const uint8_t *__restrict__ erase, uint64_t n,
                                                              uint32_t *__restrict__ tstate,
                                                              uint64_t *__restrict__ tcount) {
    __shared__ uint32_t lds[4];
    __shared__ uint64_t lds64[4];
    uint8_t w[16], er[16];
    const uint64_t p0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * 16;
    load_rows<MODE>(W, erase, n, p0, w, er);
    uint32_t s = 0;
    uint64_t kept = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (p0 + j >= n) continue;
        s = state_combine(s, row_state<MODE>(w[j], er[j] != 0));
        kept += er[j] == 0;
    }
    uint32_t total;
    (void)block_excl_scan_state(s, &total, lds);
    if (threadIdx.x == 0) tstate[blockIdx.x] = total;
    if (MODE == kErase) {
        uint64_t ktotal;
        (void)block_excl_scan(kept, &ktotal, lds64);
        if (threadIdx.x == 0) tcount[blockIdx.x] = ktotal;
    }
}

// one block: tstate / tcount -> their exclusive scans over the tiles; *out_total = the kept rows
__global__ __launch_bounds__(kThreads) void state_carry_kernel(uint32_t *__restrict__ tstate,
                                                               uint64_t *__restrict__ tcount, uint64_t ntiles,
                                                               uint64_t *__restrict__ out_total) {
    __shared__ uint32_t lds[4];
    __shared__ uint64_t lds64[4];
    uint32_t carry = 0;
    uint64_t ccarry = 0;
    for (uint64_t base = 0; base < ntiles; base += kThreads) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t x = i < ntiles ? tstate[i] : 0;
        uint32_t total;
        const uint32_t ex = block_excl_scan_state(x, &total, lds);
        if (i < ntiles) tstate[i] = state_combine(carry, ex);
        carry = state_combine(carry, total);
        if (tcount) {
            const uint64_t c = i < ntiles ? tcount[i] : 0;
            uint64_t ctotal;
            const uint64_t cex = block_excl_scan(c, &ctotal, lds64);
            if (i < ntiles) tcount[i] = ccarry + cex;
            ccarry += ctotal;
        }
    }
    if (threadIdx.x == 0 && out_total) *out_total = ccarry;
}

// single[i] = W[i] in 1..4 and the next row of its class is no minus label (is_single_incoming)
__global__ __launch_bounds__(kThreads) void single_apply_kernel(const uint8_t *__restrict__ W, uint64_t n,
                                                                const uint32_t *__restrict__ tstate,
                                                                uint8_t *__restrict__ single) {
    __shared__ uint32_t lds[4];
    uint8_t w[16], er[16];
    const uint64_t p0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * 16;
    load_rows<kSingle>(W, nullptr, n, p0, w, er);
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (p0 + j < n) s = state_combine(s, row_state<kSingle>(w[j], false));
    uint32_t total;
    uint32_t run = state_combine(tstate[blockIdx.x], block_excl_scan_state(s, &total, lds));
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (p0 + j >= n) continue;
        const uint64_t i = n - 1 - (p0 + j);
        const uint8_t x = w[j];
        single[i] = (i >= 1 && x >= 1 && x <= 4 && ((run >> (2 * x)) & 3u) != 2u) ? 1 : 0;
        run = state_combine(run, row_state<kSingle>(x, false));
    }
}

// BOSS::erase_edges.  pass 0: every kept row goes to its scanned position; a minus label whose class
// lost a plain row since its last kept row loses the minus; aux (may be null) is carried along; the
// kept rows up to each old F boundary are counted.  pass 1 (after pass 0): an erased row with `last`
// hands it to the previous kept row when that row's output index is >= 1.
__global__ __launch_bounds__(kThreads) void erase_apply_kernel(const uint8_t *__restrict__ W,
                                                               const uint8_t *__restrict__ last,
                                                               const uint8_t *__restrict__ aux,
                                                               const uint8_t *__restrict__ erase, uint64_t n,
                                                               const uint32_t *__restrict__ tstate,
                                                               const uint64_t *__restrict__ tcount, FVec f,
                                                               int pass, uint8_t *__restrict__ W_out,
                                                               uint8_t *__restrict__ last_out,
                                                               uint8_t *__restrict__ aux_out,
                                                               uint64_t *__restrict__ F_out) {
    __shared__ uint32_t lds[4];
    __shared__ uint64_t lds64[4];
    uint8_t w[16], er[16];
    const uint64_t p0 = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * 16;
    load_rows<kErase>(W, erase, n, p0, w, er);
    uint32_t s = 0;
    uint64_t kept = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (p0 + j >= n) continue;
        s = state_combine(s, row_state<kErase>(w[j], er[j] != 0));
        kept += er[j] == 0;
    }
    uint32_t total;
    uint64_t ktotal;
    uint32_t run = state_combine(tstate[blockIdx.x], block_excl_scan_state(s, &total, lds));
    uint64_t o = tcount[blockIdx.x] + block_excl_scan(kept, &ktotal, lds64);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint64_t i = p0 + j;
        if (i >= n) continue;
        const uint8_t x = w[j];
        const bool erased = er[j] != 0;
        if (pass == 1) {
            if (erased && (last[i] & 1) && o > 1 && o - 1 < n) last_out[o - 1] = 1;
            o += !erased;
            continue;
        }
        if (!erased && o < n) {
            const uint32_t c = x % 5;
            W_out[o] = (x > 5 && ((run >> (2 * c)) & 3u) == 2u) ? (uint8_t)c : x;
            last_out[o] = last[i] & 1;
            if (aux) aux_out[o] = aux[i];
        }
        run = state_combine(run, row_state<kErase>(x, erased));
        o += !erased;
#pragma unroll
        for (int c = 0; c < 5; ++c)
            if (f.F[c] == i) F_out[c] = o - 1;  // the kept rows in [1, F[c]]: row 0 is always kept
    }
}

// tstate: ntiles words, tcount: ntiles words (kErase)
inline uint64_t state_tiles(uint64_t n) { return (n + kTile - 1) / kTile; }

// ---------------------------------------------------------------- the source-dummy tree, all levels

// out[0] = the roots: rows 2 .. the first row with last == 1 (or n - 1), when n > 2 and last[1] == 0
__global__ __launch_bounds__(64) void prune_roots_kernel(Nav nav, uint64_t *__restrict__ out) {
    if (threadIdx.x != 0) return;
    uint64_t roots = 0;
    if (nav.n > 2 && !((nav.last[0] >> 1) & 1)) {
        const uint64_t before = nav.rank_last(1);
        uint64_t end = nav.last_rank[nav.nw] > before ? nav.select_last(before + 1) : nav.n - 1;
        if (end > nav.n - 1) end = nav.n - 1;
        roots = end >= 2 ? end - 1 : 0;
    }
    out[0] = roots;
}

__global__ __launch_bounds__(kThreads) void prune_root_level_kernel(uint64_t m, uint64_t *__restrict__ edge,
                                                                    uint64_t *__restrict__ parent) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    edge[t] = 2 + t;
    parent[t] = 0;
}

// One thread per edge of a level: flags it `source`; an end edge (depth k, or W % 5 == 0) gets its
// `needed`; any other gets the rows of the node it leads to (first, cnt).  W % 5 follows minus labels.
__global__ __launch_bounds__(kThreads) void prune_visit_kernel(Nav nav, const uint8_t *__restrict__ single,
                                                               const uint64_t *__restrict__ edge, uint64_t m,
                                                               int at_depth_k, uint8_t *__restrict__ source,
                                                               uint8_t *__restrict__ needed,
                                                               uint64_t *__restrict__ first,
                                                               uint32_t *__restrict__ cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    uint64_t e = edge[t];
    if (e >= nav.n) e = nav.n - 1;
    source[e] = 1;
    const uint8_t c = nav.W[e] % 5;
    if (at_depth_k || c == 0) {
        needed[t] = (c == 0 || single[e]) ? 1 : 0;
        first[t] = 0;
        cnt[t] = 0;
        return;
    }
    uint64_t le = nav.fwd(e, c);
    if (le >= nav.n) le = nav.n - 1;
    const uint64_t node = nav.rank_last(le);
    const uint64_t fe = node ? nav.select_last(node - 1) + 1 : 1;
    const uint64_t rows = le >= fe ? le - fe + 1 : 0;
    needed[t] = 0;
    first[t] = fe;
    cnt[t] = rows > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rows;
}

// the next level: the rows of every node, each with the slot of the edge that led to it
__global__ __launch_bounds__(kThreads) void prune_expand_kernel(const uint64_t *__restrict__ first,
                                                                const uint32_t *__restrict__ cnt,
                                                                const uint64_t *__restrict__ scan, uint64_t m,
                                                                uint64_t *__restrict__ next_edge,
                                                                uint64_t *__restrict__ next_parent,
                                                                uint64_t next_count) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    const uint64_t fe = first[t], o = scan[t];
    const uint32_t c = cnt[t];
    for (uint32_t j = 0; j < c && o + j < next_count; ++j) {
        next_edge[o + j] = fe + j;
        next_parent[o + j] = t;
    }
}

// a needed edge makes its parent needed (every writer stores the same 1)
__global__ __launch_bounds__(kThreads) void prune_up_kernel(const uint8_t *__restrict__ needed,
                                                            const uint64_t *__restrict__ parent, uint64_t m,
                                                            uint8_t *__restrict__ parent_needed,
                                                            uint64_t parent_count) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m || !needed[t]) return;
    const uint64_t p = parent[t];
    if (p < parent_count) parent_needed[p] = 1;
}

// redundant = visited and not needed, for rows other than 0 and 1
__global__ __launch_bounds__(kThreads) void prune_mark_kernel(const uint64_t *__restrict__ edge,
                                                              const uint8_t *__restrict__ needed, uint64_t total,
                                                              uint64_t n, uint8_t *__restrict__ erase) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= total || needed[t]) return;
    const uint64_t e = edge[t];
    if (e > 1 && e < n) erase[e] = 1;
}

}  // namespace dbgdev
}  // namespace mtg
