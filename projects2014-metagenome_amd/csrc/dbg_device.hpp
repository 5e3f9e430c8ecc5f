// dbg_device.hpp -- the per-row stages of the graph-file writer (dbg_io.hpp, sdsl_io.hpp) as HIP
// kernels over a device chunk (wave64, gfx950).  The host writer is the specification: every array
// here is what its "compute payload" half produces, bit for bit.
//
//   W  -> per-tile symbol histogram (16 bins + "other") -> scan -> the wavelet-tree node bits
//         (a row at node v sits at bv_pos[v] + #{earlier rows under v}; dbg_wt_fill_kernel)
//   bits -> rank_support_v<1> / rank_support_v5<1> words (block popcount, scan, field pack)
//   W, last -> the navigation directory of BossNav (ones of last and rows with W == c before each
//         64-row block), and rank_last / rank_W / select_last / tighten_range / fwd on it
//   -> the suffix-range index, one kernel per suffix char
//   -> the valid-edge mask, a level-synchronous walk of the source-dummy tree
//   weights -> the width-w int_vector's words
// The Huffman shape, both select supports, bit_vector_small and the framing stay host code.
//
// Bounds: every global write is indexed by a thread id below the launch's element count, by a scanned
// count that sized the buffer, or is checked against the buffer's length; reads through navigation
// results clamp the row to n - 1, so arrays that are no BOSS table cannot leave their buffers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mtg {
namespace dbgdev {

constexpr int kThreads = 256;                      // every kernel: 4 waves
constexpr int kTile = 4096;                        // rows of W per workgroup: 16 bytes per thread
constexpr int kMaxInner = 15;                      // inner nodes of a Huffman tree over 16 symbols
constexpr int kSegs = kTile / 64;                  // 64-row segments of a tile, 16 per wave
constexpr int kTileWords = kTile * kMaxInner / 64 + 2 * kMaxInner + 2;  // node spans of one tile, in words
constexpr int kScanItems = 16;                     // items per thread of the scan kernels
constexpr int kScanTile = kThreads * kScanItems;

// ------------------------------------------------------------------------------- helpers

// 16 bytes of a byte array from row i0 (one 16-byte load when whole and aligned); bytes past n are 0xFF.
// Returns the rows that exist.
__device__ inline int load16(const uint8_t *__restrict__ p, uint64_t i0, uint64_t n, uint8_t out[16]) {
    if (i0 + 16 <= n && ((uintptr_t)(p + i0) & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p + i0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) out[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        return 16;
    }
    int valid = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const bool in = i0 + j < n;
        out[j] = in ? p[in ? i0 + j : 0] : (uint8_t)0xFF;
        valid += in;
    }
    return valid;
}

__device__ inline uint64_t wave_incl_scan(uint64_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

__device__ inline uint64_t wave_sum(uint64_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor((unsigned long long)x, d, 64);
    return x;
}

// exclusive scan of one value per thread over the 256-thread block; *total = the block's sum
__device__ inline uint64_t block_excl_scan(uint64_t x, uint64_t *total, uint64_t *lds /* 4 words */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t incl = wave_incl_scan(x);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const uint64_t s = lds[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + incl - x;
}

// ---------------------------------------------------------------- exclusive scan u32 -> u64
// out[i] = in[0] + .. + in[i - 1] for i in [0, n], out[n] the total: tile sums, one block scanning the
// tile sums, then every tile rescanned from its start.

__global__ __launch_bounds__(kThreads) void scan_tile_sums_kernel(const uint32_t *__restrict__ in, uint64_t n,
                                                                  uint64_t *__restrict__ tsum) {
    __shared__ uint64_t lds[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint64_t s = 0;
    if (i0 + kScanItems <= n) {
        const uint4 *p = reinterpret_cast<const uint4 *>(in + i0);  // i0 is a multiple of 16 entries
#pragma unroll
        for (int q = 0; q < kScanItems / 4; ++q) {
            const uint4 v = p[q];
            s += (uint64_t)v.x + v.y + v.z + v.w;
        }
    } else {
        for (int j = 0; j < kScanItems; ++j)
            if (i0 + j < n) s += in[i0 + j];
    }
    uint64_t total;
    (void)block_excl_scan(s, &total, lds);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void scan_tile_offsets_kernel(uint64_t *__restrict__ tsum, uint64_t ntiles,
                                                                     uint64_t *__restrict__ out_total) {
    __shared__ uint64_t lds[4];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < ntiles; base += kThreads) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t x = i < ntiles ? tsum[i] : 0;
        uint64_t total;
        const uint64_t ex = block_excl_scan(x, &total, lds);
        if (i < ntiles) tsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *out_total = carry;
}

__global__ __launch_bounds__(kThreads) void scan_apply_kernel(const uint32_t *__restrict__ in, uint64_t n,
                                                              const uint64_t *__restrict__ tsum,
                                                              uint64_t *__restrict__ out) {
    __shared__ uint64_t lds[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint32_t v[kScanItems];
    uint64_t s = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        v[j] = i0 + j < n ? in[i0 + j] : 0;
        s += v[j];
    }
    uint64_t total;
    uint64_t run = tsum[blockIdx.x] + block_excl_scan(s, &total, lds);
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (i0 + j < n) out[i0 + j] = run;
        run += v[j];
    }
}

// tmp: ceil(n / kScanTile) words; out: n + 1 words
inline void exclusive_scan(const uint32_t *in, uint64_t n, uint64_t *out, uint64_t *tmp, hipStream_t s) {
    const uint64_t ntiles = (n + kScanTile - 1) / kScanTile;
    if (ntiles) scan_tile_sums_kernel<<<dim3((unsigned)ntiles), dim3(kThreads), 0, s>>>(in, n, tmp);
    scan_tile_offsets_kernel<<<dim3(1), dim3(kThreads), 0, s>>>(tmp, ntiles, out + n);
    if (ntiles) scan_apply_kernel<<<dim3((unsigned)ntiles), dim3(kThreads), 0, s>>>(in, n, tmp, out);
}

// out[j] = in[idx[j]] (the few scan entries the host needs)
struct GatherIdx {
    uint64_t idx[24];
};
__global__ __launch_bounds__(64) void gather_kernel(const uint64_t *__restrict__ in, GatherIdx g, int count,
                                                    uint64_t *__restrict__ out) {
    if ((int)threadIdx.x < count) out[threadIdx.x] = in[g.idx[threadIdx.x]];
}

// ---------------------------------------------------------------------- W histogram per tile

// hist[s * ntiles + tile] = rows of the tile with W == s (s < 16), row 16 = rows with W >= 16
__global__ __launch_bounds__(kThreads) void w_hist_kernel(const uint8_t *__restrict__ W, uint64_t n, uint64_t ntiles,
                                                          uint32_t *__restrict__ hist) {
    __shared__ uint32_t sh[kThreads / 64][17];
    const uint64_t tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t b[16];
    const int valid = load16(W, tile * kTile + (uint64_t)threadIdx.x * 16, n, b);
    // sixteen 16-bit counters in four words: a thread adds at most 16, a wave at most 1024
    uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, other = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j >= valid) continue;
        const uint32_t s = b[j];
        const uint64_t inc = 1ull << (16 * (s & 3));
        const uint32_t q = s >> 2;
        c0 += q == 0 ? inc : 0;
        c1 += q == 1 ? inc : 0;
        c2 += q == 2 ? inc : 0;
        c3 += q == 3 ? inc : 0;
        other += s >= 16;
    }
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    c2 = wave_sum(c2);
    c3 = wave_sum(c3);
    other = wave_sum(other);
    if (lane == 0) {
        const uint64_t c[4] = {c0, c1, c2, c3};
#pragma unroll
        for (int s = 0; s < 16; ++s) sh[wave][s] = (uint32_t)(c[s >> 2] >> (16 * (s & 3))) & 0xFFFFu;
        sh[wave][16] = (uint32_t)other;
    }
    __syncthreads();
    if (threadIdx.x < 17) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) t += sh[w][threadIdx.x];
        hist[(uint64_t)threadIdx.x * ntiles + tile] = t;
    }
}

// ------------------------------------------------------------------------ wavelet-tree fill

// the Huffman shape as the fill kernel needs it (a kernel argument: constant memory).  Inner nodes in
// the byte_tree's breadth-first order; under[j] / one[j]: the symbols below inner node j / those that
// branch to its child[1]; row_base[s] = scan entry of (symbol s, tile 0).
struct WtTable {
    uint32_t ninner;
    uint16_t under[kMaxInner];
    uint16_t one[kMaxInner];
    uint64_t bv_pos[kMaxInner];
    uint64_t row_base[16];
};

// One tile of rows -> its bits of every inner node.  Within the tile a row's position at node j is the
// rows under j in the 64-row segments before its own (counted by ballots, scanned per node) plus the
// lanes under j before it.  The tile's span of node j is assembled in LDS at its global bit offset;
// the span's interior words are stored, its first and last word (shared with the neighbouring tiles
// or nodes) are OR-ed into the zeroed output, so the result does not depend on scheduling.
__global__ __launch_bounds__(kThreads) void wt_fill_kernel(const uint8_t *__restrict__ W, uint64_t n,
                                                           uint64_t ntiles, const uint64_t *__restrict__ scan,
                                                           WtTable tb, uint64_t *__restrict__ bv,
                                                           uint64_t bv_words) {
    __shared__ uint4 sW4[kThreads];
    __shared__ uint32_t seg[kMaxInner][kSegs];  // rows under node j per segment, then their exclusive scan
    __shared__ __attribute__((aligned(8))) uint32_t bits[2 * kTileWords];
    __shared__ uint64_t gstart[kMaxInner];
    __shared__ uint32_t ncnt[kMaxInner], wbase[kMaxInner];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t tile = blockIdx.x;
    const int ninner = (int)tb.ninner;
    {
        uint8_t b[16];
        (void)load16(W, tile * kTile + (uint64_t)tid * 16, n, b);
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j >> 2] |= (uint32_t)b[j] << (8 * (j & 3));
        sW4[tid] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int i = tid; i < 2 * kTileWords; i += kThreads) bits[i] = 0;
    __syncthreads();
    const uint8_t *sW = reinterpret_cast<const uint8_t *>(sW4);
    uint8_t sym[kSegs / 4];  // this lane's row of each of the wave's 16 segments (0xFF past n)
#pragma unroll
    for (int g = 0; g < kSegs / 4; ++g) sym[g] = sW[(wave * (kSegs / 4) + g) * 64 + lane];

    for (int j = 0; j < ninner; ++j) {
        const uint32_t under = tb.under[j];
        uint32_t mine = 0;
#pragma unroll
        for (int g = 0; g < kSegs / 4; ++g) {
            const bool u = sym[g] < 16 && ((under >> (sym[g] & 15)) & 1);
            const uint32_t c = (uint32_t)__popcll(__ballot(u));
            mine = lane == g ? c : mine;
        }
        if (lane < kSegs / 4) seg[j][wave * (kSegs / 4) + lane] = mine;
    }
    __syncthreads();
    for (int j = wave; j < ninner; j += kThreads / 64) {  // kSegs == 64: one segment per lane
        const uint32_t x = seg[j][lane];
        const uint32_t incl = (uint32_t)wave_incl_scan(x);
        seg[j][lane] = incl - x;
        if (lane == 63) ncnt[j] = incl;
    }
    if (tid < ninner) {
        uint64_t st = tb.bv_pos[tid];
        const uint32_t under = tb.under[tid];
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if ((under >> s) & 1) st += scan[(uint64_t)s * ntiles + tile] - tb.row_base[s];
        gstart[tid] = st;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t acc = 0;
        for (int j = 0; j < ninner; ++j) {
            wbase[j] = acc;
            const uint32_t c = ncnt[j];
            acc += c ? (uint32_t)(((gstart[j] & 63) + c + 63) >> 6) : 0;
        }
    }
    __syncthreads();
    for (int j = 0; j < ninner; ++j) {
        const uint32_t under = tb.under[j], one = tb.one[j];
        const uint32_t boff = 64 * wbase[j] + (uint32_t)(gstart[j] & 63);
#pragma unroll
        for (int g = 0; g < kSegs / 4; ++g) {
            const uint32_t s = sym[g] & 15;
            const bool u = sym[g] < 16 && ((under >> s) & 1);
            const uint64_t m = __ballot(u);
            if (u && ((one >> s) & 1)) {
                const uint32_t pos = boff + seg[j][wave * (kSegs / 4) + g] + (uint32_t)__popcll(m & ((1ull << lane) - 1));
                atomicOr(&bits[pos >> 5], 1u << (pos & 31));
            }
        }
    }
    __syncthreads();
    const uint64_t *bits64 = reinterpret_cast<const uint64_t *>(bits);
    for (int j = 0; j < ninner; ++j) {
        const uint32_t c = ncnt[j];
        if (!c) continue;
        const uint32_t nwj = (uint32_t)(((gstart[j] & 63) + c + 63) >> 6);
        const uint64_t gw0 = gstart[j] >> 6;
        for (uint32_t i = tid; i < nwj; i += kThreads) {
            const uint64_t v = bits64[wbase[j] + i];
            if (gw0 + i >= bv_words) continue;
            if (i == 0 || i == nwj - 1) {
                if (v) atomicOr((unsigned long long *)&bv[gw0 + i], (unsigned long long)v);
            } else {
                bv[gw0 + i] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------- rank words

// One thread per block of WPB words: cnt[b] = the block's ones, bb[2 b + 1] = the in-block prefix fields.
// WPB == 8: rank_support_v<1> (the ones before words 1..7 in 9-bit fields at bits 54, 45, .., 0);
// WPB == 32: rank_support_v5<1> (the ones before words 6, 12, .., 30 in 12-bit fields at bits 48, .., 0).
// A field exists when the vector reaches its boundary (rank_v_words / rank_v5_words close the last
// block with one more field); nblocks = (nw / WPB) + 1, the last block may hold no word at all.
template <int WPB>
__global__ __launch_bounds__(kThreads) void rank_blocks_kernel(const uint64_t *__restrict__ data, uint64_t nw,
                                                               uint64_t nblocks, uint32_t *__restrict__ cnt,
                                                               uint64_t *__restrict__ bb) {
    const uint64_t b = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= nblocks) return;
    const uint64_t w0 = b * WPB;
    uint64_t sum = 0, second = 0;
#pragma unroll
    for (int i = 0; i < WPB; ++i) {
        if (i >= 1 && w0 + i <= nw) {
            if (WPB == 8) second |= sum << (63 - 9 * i);
            else if (i % 6 == 0) second |= sum << (60 - 12 * (i / 6));
        }
        if (w0 + i < nw) sum += (uint64_t)__popcll(data[w0 + i]);
    }
    cnt[b] = (uint32_t)sum;
    bb[2 * b + 1] = second;
}

__global__ __launch_bounds__(kThreads) void rank_first_kernel(const uint64_t *__restrict__ scan, uint64_t nblocks,
                                                              uint64_t *__restrict__ bb) {
    const uint64_t b = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b < nblocks) bb[2 * b] = scan[b];
}

// ------------------------------------------------------------------- navigation directory

// cnt[r * nw + b] over the 64-row blocks: r = 0 the ones of last, r = 1 + c the rows with W == c
__global__ __launch_bounds__(kThreads) void nav_count_kernel(const uint8_t *__restrict__ W,
                                                             const uint64_t *__restrict__ last, uint64_t n,
                                                             uint64_t nw, uint32_t *__restrict__ cnt) {
    const uint64_t b = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= nw) return;
    uint32_t c[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint8_t x[16];
        const int valid = load16(W, 64 * b + 16 * q, n, x);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool in = j < valid;
#pragma unroll
            for (int s = 0; s < 5; ++s) c[s] += in && x[j] == s;
        }
    }
    cnt[b] = (uint32_t)__popcll(last[b]);
#pragma unroll
    for (int s = 0; s < 5; ++s) cnt[(uint64_t)(1 + s) * nw + b] = c[s];
}

// dir[r * (nw + 1) + w] = scan[r * nw + w] - scan[r * nw], w in [0, nw]
__global__ __launch_bounds__(kThreads) void nav_dir_kernel(const uint64_t *__restrict__ scan, uint64_t nw,
                                                           uint64_t *__restrict__ dir) {
    const uint64_t w = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t r = blockIdx.y;
    if (w <= nw) dir[r * (nw + 1) + w] = scan[r * nw + w] - scan[r * nw];
}

// BossNav (dbg_io.hpp) over device arrays; the same arithmetic, rows clamped to n - 1 on reads
struct Nav {
    const uint8_t *W;
    const uint64_t *last;
    uint64_t n, k, nw;
    const uint64_t *last_rank;  // nw + 1
    const uint64_t *wrank[5];   // nw + 1 each
    uint64_t NF[5];

    __device__ uint64_t rank_last(uint64_t i) const {
        if (i == 0) return 0;
        if (i >= n) i = n - 1;
        const uint64_t e = i + 1, w = e >> 6, b = e & 63;
        return last_rank[w] + (b ? (uint64_t)__popcll(last[w] & ((1ull << b) - 1)) : 0);
    }
    __device__ uint64_t select_last(uint64_t j) const {
        if (j == 0) return 0;
        uint64_t lo = 0, hi = nw;  // last word with last_rank[w] < j
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (last_rank[mid] < j) lo = mid; else hi = mid;
        }
        uint64_t x = last[lo];
        const uint64_t r = j - last_rank[lo];
        for (uint64_t q = 1; q < r && x; ++q) x &= x - 1;
        return 64 * lo + (x ? (uint64_t)(__ffsll((unsigned long long)x) - 1) : 0);
    }
    __device__ uint64_t rank_W(uint64_t i, uint8_t c) const {
        if (i == 0) return 0;
        if (i >= n) i = n - 1;
        const uint64_t e = i + 1, b = e >> 6;
        uint64_t r = wrank[c][b];
        for (uint64_t p = 64 * b; p < e; ++p) r += W[p] == c;
        return r - (c == 0 ? 1 : 0);
    }
    __device__ bool tighten_range(uint64_t *rl, uint64_t *ru, uint8_t s) const {
        const uint64_t rk_rl = rank_W(*rl - 1, s) + 1;
        const uint64_t rk_ru = rank_W(*ru, s);
        if (rk_rl > rk_ru) return false;
        *rl = select_last(NF[s] + rk_rl - 1) + 1;
        *ru = select_last(NF[s] + rk_ru);
        return true;
    }
    __device__ uint64_t fwd(uint64_t i, uint8_t c) const { return select_last(NF[c] + rank_W(i, c)); }
    // the last char of row i's node: the largest c whose block of nodes starts before the node's rank
    __device__ uint8_t node_last_char(uint64_t i) const {
        if (i == 0) return 0;
        const uint64_t node = rank_last(i - 1) + 1;
        uint8_t c = 0;
#pragma unroll
        for (uint8_t s = 1; s < 5; ++s) c = NF[s] < node ? s : c;
        return c;
    }
    // the row of the q-th plain c of W[1..] (rank_W's inverse): a search of the directory, then the block's
    // rows; 0 when there is none
    __device__ uint64_t select_W(uint64_t q, uint8_t c) const {
        if (q == 0) return 0;
        if (c == 0) ++q;  // row 0
        uint64_t lo = 0, hi = nw;  // last block with wrank[c][b] < q
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (wrank[c][mid] < q) lo = mid; else hi = mid;
        }
        uint64_t r = q - wrank[c][lo];
        const uint64_t end = 64 * lo + 64 < n ? 64 * lo + 64 : n;
        for (uint64_t p = 64 * lo; p < end; ++p)
            if (W[p] == c && --r == 0) return p;
        return 0;
    }
    // BOSS::bwd: the plain edge into row i's node
    __device__ uint64_t bwd(uint64_t i) const {
        if (i == 0) return 0;
        if (i >= n) i = n - 1;
        const uint64_t node = rank_last(i - 1) + 1;
        const uint8_t c = node_last_char(i);
        return node > NF[c] ? select_W(node - NF[c], c) : 0;
    }
};

struct FVec {
    uint64_t F[5];
};
// out[0..4] = NF[c] = rank_last(F[c]) (recompute_NF), out[5] = select_last(1), the main dummy node's last edge
__global__ __launch_bounds__(64) void nav_nf_kernel(Nav nav, FVec f, uint64_t *__restrict__ out) {
    if (threadIdx.x < 5) out[threadIdx.x] = nav.rank_last(f.F[threadIdx.x]);
    if (threadIdx.x == 5) out[5] = nav.select_last(1);
}

// ------------------------------------------------------------------------ suffix-range index

// level 0: the one range of the empty suffix, [1, n - 1] (empty when n == 1).  A range with last == 0
// is empty, written (n, 0) as index_suffix_ranges initialises its slots.
__global__ __launch_bounds__(64) void suffix_root_kernel(uint64_t n, uint64_t *__restrict__ out) {
    if (threadIdx.x == 0) {
        out[0] = n > 1 ? 1 : n;
        out[1] = n > 1 ? n - 1 : 0;
    }
}

// one thread per (range idx, char c): slot num * (c - 1) + idx of the next level
__global__ __launch_bounds__(kThreads) void suffix_level_kernel(Nav nav, const uint64_t *__restrict__ in,
                                                                uint64_t num, uint64_t *__restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= 4 * num) return;
    const uint64_t idx = t % num;
    const uint8_t c = (uint8_t)(t / num + 1);
    uint64_t rl = in[2 * idx], ru = in[2 * idx + 1];
    const bool ok = ru != 0 && nav.tighten_range(&rl, &ru, c);
    out[2 * t] = ok ? rl : nav.n;
    out[2 * t + 1] = ok ? ru : 0;
}

// --------------------------------------------------------------------------- valid-edge mask

// One thread per frontier entry (the last edge of a node of the source-dummy tree): flags the node's
// rows and counts the edges that lead on (W in 1..4) when the walk expands this depth.
__global__ __launch_bounds__(kThreads) void mask_count_kernel(Nav nav, const uint64_t *__restrict__ frontier,
                                                              uint64_t m, int expand, uint32_t *__restrict__ cnt,
                                                              uint8_t *__restrict__ flagged) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    const uint64_t e = frontier[t];
    const uint64_t node = nav.rank_last(e);
    const uint64_t first = node ? nav.select_last(node - 1) + 1 : 1;
    uint32_t c = 0;
    for (uint64_t i = first; i <= e && i < nav.n; ++i) {
        flagged[i] = 1;
        const uint8_t w = nav.W[i];
        c += expand && w >= 1 && w <= 4;
    }
    cnt[t] = c;
}

// the next frontier: entry scan[t] + (rank of the edge among the node's expanding edges)
__global__ __launch_bounds__(kThreads) void mask_expand_kernel(Nav nav, const uint64_t *__restrict__ frontier,
                                                               uint64_t m, const uint64_t *__restrict__ scan,
                                                               uint64_t *__restrict__ next, uint64_t next_count) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    const uint64_t e = frontier[t];
    const uint64_t node = nav.rank_last(e);
    const uint64_t first = node ? nav.select_last(node - 1) + 1 : 1;
    uint64_t o = scan[t];
    for (uint64_t i = first; i <= e && i < nav.n; ++i) {
        const uint8_t w = nav.W[i];
        if (w >= 1 && w <= 4 && o < next_count) next[o++] = nav.fwd(i, w);
    }
}

// valid[i] = !(i == 0 || flagged[i] || (i >= 2 && W[i] == 0)), one word per thread; *n_valid += the set bits
__global__ __launch_bounds__(kThreads) void mask_pack_kernel(const uint8_t *__restrict__ W,
                                                             const uint8_t *__restrict__ flagged, uint64_t n,
                                                             uint64_t nw, uint64_t *__restrict__ words,
                                                             unsigned long long *__restrict__ n_valid) {
    const uint64_t w = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint64_t v = 0;
    if (w < nw) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint8_t x[16], f[16];
            const uint64_t i0 = 64 * w + 16 * q;
            const int valid = load16(W, i0, n, x);
            (void)load16(flagged, i0, n, f);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint64_t i = i0 + j;
                const bool dummy = i == 0 || f[j] != 0 || (i >= 2 && x[j] == 0);
                if (j < valid && !dummy) v |= 1ull << (16 * q + j);
            }
        }
        words[w] = v;
    }
    const uint64_t s = wave_sum((uint64_t)__popcll(v));
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(n_valid, (unsigned long long)s);
}

// ----------------------------------------------------------------------------- weights packing

// one 64-bit word of the width-w int_vector per thread (w in 1..32; values masked to w bits)
__global__ __launch_bounds__(kThreads) void weights_pack_kernel(const uint32_t *__restrict__ weights, uint64_t n,
                                                                unsigned w, uint64_t nwords,
                                                                uint64_t *__restrict__ words) {
    const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= nwords) return;
    const uint64_t mask = (1ull << w) - 1, lo = 64 * q, hi = lo + 64;
    uint64_t v = 0;
    for (uint64_t i = lo / w; i < n && i * w < hi; ++i) {
        const uint64_t x = (uint64_t)weights[i] & mask, pos = i * w;
        v |= pos >= lo ? x << (pos - lo) : x >> (lo - pos);
    }
    words[q] = v;
}

}  // namespace dbgdev
}  // namespace mtg
