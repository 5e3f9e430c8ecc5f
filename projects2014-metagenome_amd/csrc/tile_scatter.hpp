// tile_scatter.hpp -- a tile's keys, held in registers, delivered to their buckets: the step the five
// partition kernels share (extract_partition_kernel, extract_partition_fast_kernel,
// extract_partition_fast2_kernel, msd_partition_kernel, rc_partition_gapped_kernel).  Device code only.
//
//   1  (kernel)  count the tile's keys per bucket with LDS atomics; each key keeps its rank r in its bucket
//   2+3 tile_reserve_runs   the counts become in-tile offsets; one 64-bit atomic per non-empty bucket
//                           reserves the bucket's run at its cursor
//       __syncthreads()     (kernel)
//   4  (kernel)  scatter the keys into the LDS tile at s_off[bucket] + r
//   5  tile_publish_runs    check each run against its bucket's end, publish its base in s_gbase
//       __syncthreads()     (kernel)
//   6  tile_write_runs      a strided loop over the staged tile writes key p to
//                           s_gbase[bucket] + (p - s_off[bucket])
//
// Steps 1 and 4 stay in the kernels: they sit between the kernel's own register arrays (keys, counts,
// validity mask or rank sentinel).  Each kernel declares its own __shared__ arrays and passes pointers
// in, its aliasing included; the cursors and ends are a small policy object, the bucket of a key, what an
// overflow raises and the final store small lambdas, all passed by value.
#pragma once

#include "device_common.hpp"

namespace mtg {

// what steps 2+3 return: a thread's PER buckets, kept for step 5, and the tile's key count
template <int PER>
struct TileRuns {
    uint32_t c[PER];            // the tile's keys in the bucket
    unsigned long long g[PER];  // the reserved run's base (0: an empty bucket)
    unsigned long long e[PER];  // the bucket's end (unused without ends)
    uint32_t total;             // the tile's key count (the same in every thread)
};

// Where a tile's buckets live in global memory is one small policy per kernel: cursor(i) is the index
// of bucket i's cursor, checked() says whether the buckets have ends (a constant, or the kernel's runtime
// test of its bend pointer) and end(i, ci) loads bucket i's, ci being its cursor's index.
// PlainBuckets: one cursor per bucket and no ends (the histogram pass counted exactly these keys).
struct PlainBuckets {
    __device__ __forceinline__ size_t cursor(uint32_t i) const { return i; }
    __device__ __forceinline__ constexpr bool checked() const { return false; }
    __device__ __forceinline__ unsigned long long end(uint32_t, size_t) const { return 0; }
};
struct NoRaise {
    __device__ __forceinline__ void operator()() const {}
};

// Steps 2+3: thread t owns buckets t * PER .. t * PER + PER - 1 of the nb (<= BLOCK * PER).  Reads their
// counts from s_cnt, writes the buckets' offsets in the tile to s_off and reserves the run of each
// non-empty bucket at cursor[at.cursor(i)]; the bucket's end, where there are ends, is loaded next to
// the atomic.  The reservations are issued here and consumed in tile_publish_runs, after the
// kernel's LDS scatter, so their round trip to the cursors overlaps the scatter instead of stalling the
// workgroup before it.
// Off: u32, or u16 where TILE <= 65536 (the kernel asserts it).  s_off may be s_cnt itself; then
// COUNTS_BARRIER must be set: every count is read before the offsets overwrite them.
template <int BLOCK, int PER, bool COUNTS_BARRIER, typename Off, typename Buckets>
__device__ __forceinline__ TileRuns<PER> tile_reserve_runs(const uint32_t *s_cnt, Off *s_off, uint32_t *s_scan,
                                                           uint32_t nb, unsigned long long *cursor, Buckets at) {
    TileRuns<PER> t;
    const uint32_t tid = threadIdx.x;
    uint32_t sum = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t i = tid * PER + q;
        t.c[q] = i < nb ? s_cnt[i] : 0;
        sum += t.c[q];
    }
    uint32_t total;
    uint32_t off = block_exclusive_sum<BLOCK>(sum, s_scan, &total);
    if (COUNTS_BARRIER) __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t i = tid * PER + q;
        t.g[q] = 0, t.e[q] = 0;
        if (i < nb) {
            s_off[i] = (Off)off;
            const size_t ci = at.cursor(i);
            if (t.c[q]) {
                t.g[q] = atomicAdd(&cursor[ci], (unsigned long long)t.c[q]);
                if (at.checked()) t.e[q] = at.end(i, ci);
            }
        }
        off += t.c[q];
    }
    t.total = total;
    return t;
}

// Step 5, after the LDS scatter: bucket i's run base goes to s_gbase[i].  The ends are exact ones from
// pass A's histogram, or speculative ones sized from a sample.  A run reaching past its bucket's end --
// pass A counted this bucket differently: never; a speculative bucket too small -- is not written
// (base ~0) and raise() tells the host, which stops or runs the exact passes instead.
// bdelta (the collect rounds' one pass B; may be null): bucket i's keys go bdelta[i] elements away from
// their layout position, each round's buckets into that round's buffer.
template <int PER, typename Buckets, typename Raise = NoRaise>
__device__ __forceinline__ void tile_publish_runs(const TileRuns<PER> &t, uint32_t nb, Buckets at,
                                                  unsigned long long *s_gbase, Raise raise = Raise{},
                                                  const long long *bdelta = nullptr) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t i = tid * PER + q;
        if (i < nb) {
            unsigned long long g = t.g[q];
            if (at.checked() && t.c[q] && g + t.c[q] > t.e[q]) {
                raise();
                g = ~0ull;
            } else if (bdelta) {
                g += (unsigned long long)bdelta[i];
            }
            s_gbase[i] = g;
        }
    }
}

// Step 6, after a barrier: the staged tile (total keys, bucket by bucket) goes out as one run per bucket:
// store(o, key, p) writes key, staged at p, to element o.  Runs without a base are skipped.
template <int BLOCK, typename KeyT, typename Off, typename Buckets, typename BucketOf, typename Store>
__device__ __forceinline__ void tile_write_runs(const KeyT *s_keys, const Off *s_off, const unsigned long long *s_gbase,
                                                uint32_t total, Buckets at, BucketOf bucket_of, Store store) {
    for (uint32_t p = threadIdx.x; p < total; p += BLOCK) {
        const KeyT key = s_keys[p];
        const uint32_t lb = bucket_of(key);
        if (at.checked() && s_gbase[lb] == ~0ull) continue;
        store(s_gbase[lb] + (p - s_off[lb]), key, p);
    }
}

}  // namespace mtg
