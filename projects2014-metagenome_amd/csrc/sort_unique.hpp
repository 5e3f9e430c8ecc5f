// sort_unique.hpp -- host drivers of the sort + unique stages: the LSD onesweep sort, the MSD sort with
// its speculative levels and the fused rc merge (kernels in radix_sort.hpp, msd_sort.hpp and
// boss_kernels.hpp), and the tiled merge of two sorted arrays.  Included by boss_pipeline.hip only.
#pragma once

#include "ctx.hpp"

namespace mtg {

// starts[0..n] = exclusive scan of counts[0..n) (msd_sort.hpp: scan_counts_kernel, one look-back launch);
// cursors: starts[0..n) written there too
static void scan_counts(Ctx &c, const uint32_t *counts, uint64_t n, uint64_t *starts,
                        unsigned long long *cursors = nullptr) {
    uint32_t ep;
    const uint64_t st = ceil_div(n, 4096);
    uint64_t *desc = acquire_desc(c, st, &ep);
    HIP_CHECK(hipMemsetAsync(&c.small->counter, 0, 4, c.stream));
    scan_counts_kernel<<<dim3((unsigned)st), dim3(512), 0, c.stream>>>(counts, n, starts, desc, ep,
                                                                      &c.small->counter, &c.small->error, cursors);
    HIP_CHECK(hipGetLastError());
}

// the same, then the total read back (a host sync)
static uint64_t scan_counts_total(Ctx &c, const uint32_t *counts, uint64_t n, uint64_t *starts,
                                  unsigned long long *cursors = nullptr) {
    scan_counts(c, counts, n, starts, cursors);
    return read_u64(c, (const unsigned long long *)(starts + n));
}

// bucket index of a sorted key array (boss_kernels.hpp: bucket_index_kernel + the grid-wide fill of
// its long empty runs)
constexpr uint32_t kBucketRuns = 4096;
template <int L>
static void bucket_index(Ctx &c, const Key<L> *keys, uint64_t n, unsigned shift, uint64_t nb, uint64_t *start) {
    uint64_t *runs = (uint64_t *)c.ws.get(Workspace::BRUNS, kBucketRuns * 24);
    HIP_CHECK(hipMemsetAsync(&c.small->bruns, 0, 4, c.stream));
    const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(n + 1, 256), 8192));
    bucket_index_kernel<L><<<dim3((unsigned)g), dim3(256), 0, c.stream>>>(keys, n, shift, nb, start, runs,
                                                                         &c.small->bruns, kBucketRuns);
    HIP_CHECK(hipGetLastError());
    bucket_fill_kernel<<<dim3(1024), dim3(256), 0, c.stream>>>(runs, &c.small->bruns, kBucketRuns, start);
    HIP_CHECK(hipGetLastError());
}

// exclusive scans of the per-pass digit counts: block p scans hist[p * 256 ..] into start[p * 256 ..]
__global__ __launch_bounds__(256) void digit_starts_kernel(const unsigned long long *__restrict__ hist,
                                                           uint64_t *__restrict__ start) {
    __shared__ uint64_t s_wsum[4];
    const uint32_t t = threadIdx.x, p = blockIdx.x;
    const uint64_t v = hist[p * 256 + t];
    uint64_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(x, o, 64);
        if ((t & 63) >= (uint32_t)o) x += y;
    }
    if ((t & 63) == 63) s_wsum[t >> 6] = x;
    __syncthreads();
    uint64_t before = 0;
    for (uint32_t w = 0; w < (t >> 6); ++w) before += s_wsum[w];
    start[p * 256 + t] = before + x - v;
}

// LSD radix sort of keys[0..n) (and vals) over the low nbits; result left in *keys / *vals
// (pointers swapped with *alt / *valt as passes ping-pong).  Passes whose digit is the same for every key
// are skipped.  spec_first: the lowest pass is launched before the histogram reaches the host (the digit
// starts are scanned on the device), so the copy and the host's look at it overlap that pass -- for
// inputs whose lowest digit is never constant (the dense dummy ranks); a constant one costs one pass.
template <int L, bool HAS_VAL>
static void radix_sort(Ctx &c, Key<L> **keys, Key<L> **alt, uint32_t **vals, uint32_t **valt,
                       uint64_t n, unsigned nbits, bool stats, bool spec_first = false) {
    if (n < 2) return;
    const int passes = (int)ceil_div(nbits, 8);
    auto *hist = (unsigned long long *)c.ws.get(Workspace::HIST, passes * 256 * 8);
    HIP_CHECK(hipMemsetAsync(hist, 0, passes * 256 * 8, c.stream));
    const uint64_t hgrid = std::min<uint64_t>(ceil_div(n, 256), 4096);
    radix_histogram_kernel<L><<<dim3((unsigned)hgrid), dim3(256), 0, c.stream>>>(*keys, n, passes, hist);
    HIP_CHECK(hipGetLastError());
    auto *dstart = (uint64_t *)c.ws.get(Workspace::STARTS_DIGIT, passes * 256 * 8);
    digit_starts_kernel<<<dim3((unsigned)passes), dim3(256), 0, c.stream>>>(hist, dstart);
    HIP_CHECK(hipGetLastError());
    std::vector<unsigned long long> h(passes * 256);
    HIP_CHECK(hipMemcpyAsync(h.data(), hist, h.size() * 8, hipMemcpyDeviceToHost, c.stream));
    constexpr int TILE = SortTraits<L>::TILE;
    const uint64_t tiles = ceil_div(n, TILE);
    if (tiles > 0xFFFFFFFFull) throw std::runtime_error("sort too large");
    EventTimer tm(c.stream);
    std::vector<int> done;
    auto launch = [&](int p) {
        uint32_t epoch;
        uint64_t *desc = acquire_desc(c, tiles * 256, &epoch);
        HIP_CHECK(hipMemsetAsync(&c.small->counter, 0, 4, c.stream));
        tm.mark();
        onesweep_kernel<L, HAS_VAL><<<dim3((unsigned)tiles), dim3(SortTraits<L>::BLOCK), 0, c.stream>>>(
            *keys, *alt, HAS_VAL ? *vals : nullptr, HAS_VAL ? *valt : nullptr, n, 8u * p,
            dstart + p * 256, desc, epoch, &c.small->counter, &c.small->error);
        HIP_CHECK(hipGetLastError());
        tm.mark();
        std::swap(*keys, *alt);
        if (HAS_VAL) std::swap(*vals, *valt);
        done.push_back(p);
    };
    if (spec_first) launch(0);
    HIP_CHECK(hipStreamSynchronize(c.stream));  // the histogram on the host (`h` is a local)
    for (int p = spec_first ? 1 : 0; p < passes; ++p) {
        bool trivial = false;
        for (int d = 0; d < 256; ++d)
            if (h[p * 256 + d] == n) trivial = true;
        if (!trivial) launch(p);
    }
    if (stats && !done.empty()) {
        HIP_CHECK(hipStreamSynchronize(c.stream));
        for (size_t i = 0; i < done.size(); ++i) c.build.radix_ms += tm.ms(2 * i, 2 * i + 1);
        c.build.radix_launches += done.size();
        c.build.radix_bytes += (double)done.size() * 2.0 * n * (sizeof(Key<L>) + (HAS_VAL ? 4 : 0));
    }
}

__global__ void set_u64_kernel(uint64_t *p, uint64_t a) { *p = a; }

// p[i] = v for i in [lo, hi)
__global__ __launch_bounds__(256) void fill_u64_kernel(uint64_t *__restrict__ p, uint64_t lo, uint64_t hi, uint64_t v) {
    const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += T) p[i] = v;
}

__global__ void set_pair_kernel(uint64_t *p, uint64_t a, uint64_t b) {
    p[0] = a;
    p[1] = b;
}

// Duplication estimate for the MSD plan: m evenly spaced sample keys go into a hash table of
// 64-bit fingerprints; the number of samples that find their fingerprint already present is
// C ~ m^2 / (2 n) * E_w[mult] (E_w: multiplicity seen by a random occurrence).  Reads arrive in
// random genome order, so evenly spaced samples are as good as random ones.
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

template <int L>
__global__ void dup_sample_kernel(const Key<L> *__restrict__ keys, uint64_t n, uint32_t m,
                                  unsigned long long *__restrict__ table, uint32_t mask,
                                  unsigned long long *__restrict__ hits) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const Key<L> k = keys[(uint64_t)((double)j * ((double)n / m))];
    uint64_t h = 0x9e3779b97f4a7c15ull;
#pragma unroll
    for (int i = 0; i < L; ++i) h = mix64(h ^ k.w[i]);
    h |= 1;  // 0 marks an empty slot
    uint32_t slot = (uint32_t)(h >> 32) & mask;
    while (true) {
        const unsigned long long prev = atomicCAS(&table[slot], 0ull, (unsigned long long)h);
        if (prev == 0) return;
        if (prev == h) {
            atomicAdd(hits, 1ull);
            return;
        }
        slot = (slot + 1) & mask;
    }
}

// expected copies per distinct key of keys[0..n), conservative (it may err low, which costs a
// planned bit, never an overflowing plan); `fallback` below the sampling size
template <int L>
static double estimate_dup(Ctx &c, const Key<L> *keys, uint64_t n, double fallback) {
    constexpr uint32_t M = 1u << 20, SLOTS = 1u << 22;
    if (n < 8ull * M) return fallback;
    unsigned long long *table = (unsigned long long *)c.ws.get(Workspace::DUP_TABLE, (SLOTS + 1) * 8ull);
    HIP_CHECK(hipMemsetAsync(table, 0, (SLOTS + 1) * 8ull, c.stream));
    dup_sample_kernel<L><<<dim3(M / 256), dim3(256), 0, c.stream>>>(keys, n, M, table, SLOTS - 1, table + SLOTS);
    HIP_CHECK(hipGetLastError());
    const double hits = (double)read_u64(c, table + SLOTS);
    const double ew = 2.0 * (double)n * hits / ((double)M * M);  // E_w[multiplicity]
    const double dup = std::max(1.0, ew / 1.2);  // E_w / mean: 1.17 at 10x, 1.29 at 1.25x
    if (c.knobs.debug) fprintf(stderr, "[mtg debug] dup estimate n=%lu hits=%.0f E_w=%.2f -> %.2f\n", (unsigned long)n, hits, ew, dup);
    return dup;
}

// Sort + unique (+ saturating count merge) of keys[0..n) over their low nbits by MSD
// partitioning and per-group LDS hashing (msd_sort.hpp).  `dup` is the expected number of
// copies per distinct key, used only to plan the partition depth; a wrong guess costs time,
// never correctness (overflowing groups take another level or the LSD fallback).
// Result: sorted distinct keys in *keys (counts in *vals); returns their number.
struct MsdPlan {
    unsigned levels;
    unsigned digit_end[4];  // cumulative significant bits after each level
};

// partition depth: enough top bits T that an average final bucket holds <= LIMIT/3 distinct
// keys (canonical k-mers are up to 2x denser at small prefixes), in levels of <= max_digit
// bits (one full read + scatter each)
constexpr double kPlanDiv = 2.5;  // planned distinct keys per final bucket = LIMIT / kPlanDiv

template <int L>
static MsdPlan msd_plan(const Ctx &c, uint64_t n, unsigned nbits, double dup) {
    const double LIMIT = (double)LocalTraits<L>::LIMIT / 2;  // half-size LDS tables
    const unsigned dmax = MSD_DBITS;
    unsigned T = 0;
    while (T < nbits && T < 3 * dmax && (double)n / dup / (double)(1ull << T) > LIMIT / kPlanDiv)
        ++T;
    MsdPlan p{};
    p.levels = (T + dmax - 1) / dmax;
    if (c.knobs.min_levels > p.levels && T >= c.knobs.min_levels) p.levels = c.knobs.min_levels;  // (tests: MTG_MSD_LEVELS)
    for (unsigned l = 1; l <= p.levels; ++l) p.digit_end[l] = T * l / p.levels;
    return p;
}

// a plan of T bits whose level 1 is fixed at b1 bits (its producer's digit: the fused K1's pass B, the
// routed collect's routing digit), the rest split evenly over the fewest later levels
static MsdPlan level1_fixed_plan(unsigned b1, unsigned T) {
    MsdPlan q{};
    q.levels = 1 + (T - b1 + MSD_DBITS - 1) / MSD_DBITS;
    q.digit_end[1] = b1;
    for (unsigned l = 2; l <= q.levels; ++l) q.digit_end[l] = b1 + (T - b1) * (l - 1) / (q.levels - 1);
    return q;
}

// The plan of the rc sort fused with the merge (and of the canonical set's bucket index it reads): u128 keys
// take one final bit fewer than the unique's plan, so a merge group holds ~480 rc + ~480 canonical keys in
// its 1024-key LDS arrays instead of ~240 + 240 -- the per-group cost (barriers, table setup) then spreads
// over twice the keys (configs[2]: 2.03e9 rc keys over 2^22 buckets, not 2^23)
template <int L>
static MsdPlan rc_plan(const Ctx &c, uint64_t n, unsigned nbits) {
    return msd_plan<L>(c, L == 2 && c.knobs.rc_wide ? std::max<uint64_t>(1, n / 2) : n, nbits, 1.0);
}

// the rc sort's local pass fused with the merge into the real edges (local_merge_kernel)
template <int L>
struct RcMerge {
    const Key<L> *ck;   // the sorted canonical set
    const uint32_t *cv;
    uint64_t nc;
    Key<L> *out;        // the real edges: merge(canonical, sorted rc)
    uint32_t *outc;
    bool done = false;  // set when the fused pass ran (else the caller merges)
    uint64_t *istart = nullptr;  // also the dummy stage's bucket index over the top ib bits of out
    unsigned ib = 0;
    GroupIndex cidx;  // the canonical set's bucket index, when its collect left one (BuildState::gidx)
};

// a batched collect round's share of the canonical set's bucket index (collect_rounds_fused): the
// speculative final level's gather writes entries [lo, hi) of `start` (2^bits buckets) as positions
// + off in the whole set
struct RoundIndex {
    uint64_t *start = nullptr;
    unsigned bits = 0;
    uint64_t off = 0, lo = 0, hi = 0;
};

// a padded input: n positions, tile t of the next level's tiling holding keys in its first tv[t]
// positions (the speculative level-1 layout of the fused K1, or a speculative middle level's output);
// [lo, hi): the previous-level buckets its keys occupy (0 / 0: unknown, every bucket).  n == 0: compact
struct PaddedLayout {
    uint64_t n = 0;
    const uint32_t *tv = nullptr;
    uint64_t lo = 0, hi = 0;
};

// Everything msd_sort_unique is told beyond the keys and their plan hints, and everything it hands back
// beyond the distinct count.  A default request is the plain sort + unique into *keys.
template <int L>
struct SortRequest {
    // hist1: counts of the top plan.digit_end[1] bits of the input, when its producer made them;
    // level1_done: the producer already scattered the keys by the plan's level-1 digit
    // (extract_partition_kernel); hist1 holds that level's counts
    const uint32_t *hist1 = nullptr;
    bool level1_done = false;
    bool distinct = false;  // the input has no duplicates (the local pass skips its hash table)
    // the input is runs->size() - 1 sorted runs at these offsets (one gather replaces the partition passes)
    const std::vector<uint64_t> *runs = nullptr;
    RcMerge<L> *rm = nullptr;  // the rc sort: its local pass fused with the merge into the real edges
    // the caller fixed the digits (the routed multi-GPU collect: level 1 is the routing digit)
    const MsdPlan *force_plan = nullptr;
    PaddedLayout gap1;  // level1_done: the padded level-1 layout the producer left (fused_pass_b_spec)
    bool track_partition = false;  // time the sort's first msd_partition launch (BuildState::radix_ms)
    bool want_gidx = false;        // the output feeds the fused rc merge: hand back its bucket index (gidx)
    bool defer_gather = false;     // ... and the set may stay in its speculative buckets (gap)
    // where the final gather writes the compact distinct keys (and counts) instead of *keys (the exchange
    // pieces and the collect rounds append each sort's keys in place); *keys then points there
    void *out = nullptr;
    uint32_t *out_vals = nullptr;
    uint64_t out_cap = ~0ull;  // keys `out` holds (more distinct keys: the usual gather into *keys)
    RoundIndex ridx;
    // a free buffer the speculative final level of a 3-level sort may partition into (the batched
    // collect's level-1 array, sized for it, free once level 2 has moved the keys out): no third block
    void *spec_into = nullptr;
    uint64_t spec_into_bytes = 0;
    // a 3-level sort's speculative middle level (spec_mid_level) partitions into this buffer (the batched
    // collect's KB, sized for it)
    void *spec_mid_into = nullptr;
    uint64_t spec_mid_bytes = 0;

    // results
    bool ridx_written = false;  // the gather wrote ridx's entries
    GroupIndex gidx;            // want_gidx: the output's bucket index, when every group was one bucket
    GappedSet gap;              // defer_gather: the output left in bucket layout (gidx indexes it compact)
};

// bucket capacities of the speculative final level: the sampled count scaled up, 20 % + 512 keys
// of slack (a bucket of ~4600 keys overflows with probability ~1e-10 at a 1/8 sample)
// (buckets outside [blo, bhi) -- below the input's first or above its last previous-level prefix --
// hold no key and get no slack: a round of a batched collect fills a fraction of the buckets)
// align (a speculative middle level, the rc sort's level 1): capacities rounded up to whole tiles of the
// next level's tiling
// tiny (tests force the overflow fallback): half the estimate, rounded down to whole tiles under align, so
// that the rounding never makes room for the other half
__global__ void spec_caps_kernel(const uint32_t *__restrict__ sample, uint64_t nb, uint32_t stride,
                                 uint32_t *__restrict__ cap, bool tiny, uint64_t blo, uint64_t bhi,
                                 uint32_t align = 0) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    if (b < blo || b >= bhi) {
        cap[b] = 0;
        return;
    }
    uint32_t v = tiny ? (uint32_t)(((uint64_t)sample[b] * stride) / 2)
                      : (uint32_t)(((uint64_t)sample[b] * stride * 6) / 5) + 512u;
    if (align) v = (tiny ? v : v + align - 1) / align * align;
    cap[b] = v;
}

// the tile fill of a speculative middle level's output (tile-aligned buckets [bstart[b], bstart[b + 1]),
// keys up to cur[b]): tile t holds keys in its first tv[t] positions -- the padded-input convention of
// the next level's kernels (PaddedLayout::tv).  ntv: the tiles tv holds, where the caller sized it before
// the buckets' total was known (the rc sort's speculative level 1)
__global__ void spec_tile_fill_kernel(const uint64_t *__restrict__ bstart, const unsigned long long *__restrict__ cur,
                                      uint64_t nb, uint32_t tile, uint32_t *__restrict__ tv, uint64_t ntv = ~0ull) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint64_t s = bstart[b], e = bstart[b + 1], k = cur[b];
    for (uint64_t t = s / tile; t < min(e / tile, ntv); ++t) {
        const uint64_t t0 = t * tile;
        tv[t] = (uint32_t)(k <= t0 ? 0 : min<uint64_t>(tile, k - t0));
    }
}

// The final MSD level of the main sort (level 2 after the fused K1's level 1) without its exact
// histogram pass (msd_hist_kernel reads all N keys: 1.68 ms at configs[1]): the buckets are sized
// from a histogram of every 8th tile with slack, the partition writes into them (a reservation past
// a bucket's end is refused and flagged), and every bucket is one local_unique group whose keys end
// where its cursor stopped.  Returns the distinct count with the sorted keys in *keys, or ~0 when
// it does not apply (too little free HBM for the two slack-sized buffers) or a bucket or a group
// overflowed -- then nothing the caller needs was touched and it runs the exact level.
// spec_counts_kernel: the keys each speculative bucket received (its cursor minus its start)
__global__ void spec_counts_kernel(const uint64_t *__restrict__ bstart, const unsigned long long *__restrict__ cur,
                                   uint64_t nb, uint32_t *__restrict__ cnt) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nb) cnt[b] = (uint32_t)(cur[b] - bstart[b]);
}

// one workgroup per bucket over buckets [lo, hi), in launches of at most 2^22 workgroups (a grid holds
// fewer than 2^32 work-items: 2^23 buckets of 512 threads do not launch at once)
template <typename F>
static void bucket_pieces(uint64_t lo, uint64_t hi, F &&launch) {
    constexpr uint64_t CH = 1ull << 22;
    for (uint64_t g0 = lo; g0 < hi; g0 += CH) launch(g0, (unsigned)std::min(CH, hi - g0));
}

// the deferred gather of a canonical set left in bucket layout (BuildState::gap), for a consumer that reads
// it compact
static void ensure_compact(Ctx &c) {
    if (!c.build.gap.valid) return;
    c.build.gap.valid = false;
    if (!c.build.gap.nb) return;
    bucket_pieces(0, c.build.gap.nb, [&](uint64_t g0, unsigned cnt) {
        group_gather_kernel<1, false><<<dim3(cnt), dim3(256), 0, c.stream>>>(
            (const Key<1> *)c.build.gap.keys, nullptr, c.build.gap.bstart, c.build.gap.ustart, (Key<1> *)c.build.gap.dst, nullptr, nullptr, 0,
            nullptr, nullptr, g0);
        HIP_CHECK(hipGetLastError());
    });
}

// rm (the rc sort fused with the merge, distinct input): the same buckets go to local_merge_kernel,
// one bucket per group, each group's output after the canonical keys before its bucket (cidx, the
// canonical sort's bucket index) and the rc keys the buckets before it received.
template <int L, bool COUNTED>
static uint64_t spec_final_level(Ctx &c, Key<L> **keys, uint32_t **vals, uint64_t n, unsigned nbits, unsigned bp,
                                 unsigned bb, uint32_t cmax, SortRequest<L> &rq, PaddedLayout &pad, bool fine = false,
                                 Key<L> *spare = nullptr) {
    // pad: the sort's input when it is still padded (msd_sort_unique), compact again once this level succeeds
    // spare (rq.spec_into, uncounted): a free buffer of rq.spec_into_bytes the buckets may take instead of SPEC_A
    // COUNTED: the counts travel with their keys (SPEC_AC / SPEC_BC) and add with saturation in the
    // local pass, as in the exact level (configs[4]'s counted route)
    if constexpr (L != 1) {
        return ~0ull;
    } else {
        constexpr double KB = COUNTED ? 12.0 : 8.0;  // bytes of a key and its count
        const bool distinct = rq.distinct;
        RcMerge<L> *const rm = rq.rm;
        if (distinct != (rm != nullptr)) return ~0ull;  // the plain unique, or the fused rc merge
        if (rm && !c.knobs.spec_rc) return ~0ull;
        const GroupIndex cidx = rm ? rm->cidx : GroupIndex{};
        if (rm && !(cidx.keys == (const void *)rm->ck && cidx.n == rm->nc && cidx.bits == bb && cidx.nbits == nbits &&
                    bb <= 32 && (!rm->istart || rm->ib >= bb)))
            return ~0ull;
        constexpr uint32_t SS = 8;
        constexpr int TILE = MsdTraits<L>::TILE;
        // after a speculative level-1 layout the input is the padded array (pad): the fused K1's, or the rc
        // sort's own (stage_rc)
        const bool g1 = bp && pad.n;
        const uint64_t npos = g1 ? pad.n : n;
        const uint32_t *tv = g1 ? pad.tv : nullptr;
        const uint64_t tiles = ceil_div(npos, TILE);
        if (c.knobs.use_lsd || !c.knobs.spec_final || tiles < 64 * SS || bb - bp > 9 || bb > 24) return ~0ull;
        // a padded input samples every tile: its tiles' fills differ (segment tails, empty tiles), so a
        // tile-granular sample sized the buckets badly (overflow at 2 M reads)
        if (g1) fine = true;
        const uint64_t nb = 1ull << bb;
        // the deferred gather (the fused rc merge follows) leaves the distinct keys in their own buckets
        // (SPEC_B); otherwise the local unique writes over its input buckets (in place: one buffer)
        const bool gap_out = !COUNTED && rq.defer_gather && c.knobs.defer_gather && rq.want_gidx;
        const bool inplace = !rm && c.knobs.spec_inplace && !gap_out;
        if (COUNTED) spare = nullptr;
        // the slack-sized buffers must fit next to everything else
        if (!spare) {
            const uint64_t fr = c.ws.free_bytes();
            if ((double)n * KB * 1.4 * (inplace ? 1.0 : 2.0) > 0.5 * (double)fr + (double)c.ws.held_slot(Workspace::SPEC_A) +
                                                  (double)c.ws.held_slot(Workspace::SPEC_B) +
                                                  (double)c.ws.held_slot(Workspace::SPEC_AC) +
                                                  (double)c.ws.held_slot(Workspace::SPEC_BC))
                return ~0ull;
        }
        uint32_t *h = (uint32_t *)c.ws.get(Workspace::MSD_COUNTS, nb * 4);
        HIP_CHECK(hipMemsetAsync(h, 0, nb * 4, c.stream));
        // 2 levels: every 8th tile (level-1 buckets span hundreds of tiles); 3 levels: the first 1/8 of every
        // tile (level-2 buckets can be only a few tiles long, and a tile-granular sample missed them)
        constexpr uint32_t GT = 8;  // fine sample: tiles per workgroup (one LDS window flush)
        msd_hist_kernel<L><<<dim3((unsigned)(fine ? ceil_div(tiles, GT) : ceil_div(tiles, SS))), dim3(MSD_BLOCK), 0,
                             c.stream>>>(*keys, npos, nbits, bb, bp, h, fine ? 1 : SS, fine ? SS : 1, fine ? GT : 1, tv);
        HIP_CHECK(hipGetLastError());
        // the buckets the keys can occupy: those under the previous level's first and last prefix
        // (a padded input's ends are not keys: every bucket)
        uint64_t blo = 0, bhi = nb;
        if (g1 && pad.hi > pad.lo) {  // a speculative middle level's output: its key range is known
            blo = pad.lo << (bb - bp);
            bhi = std::min<uint64_t>(nb, pad.hi << (bb - bp));
        } else if (bp && !g1) {
            Key<L> ends[2];
            HIP_CHECK(hipMemcpyAsync(&ends[0], *keys, sizeof(Key<L>), hipMemcpyDeviceToHost, c.stream));
            HIP_CHECK(hipMemcpyAsync(&ends[1], *keys + (n - 1), sizeof(Key<L>), hipMemcpyDeviceToHost, c.stream));
            HIP_CHECK(hipStreamSynchronize(c.stream));
            blo = (ends[0].w[0] >> (nbits - bp)) << (bb - bp);
            bhi = std::min<uint64_t>(nb, ((ends[1].w[0] >> (nbits - bp)) + 1) << (bb - bp));
        }
        uint32_t *cap = (uint32_t *)c.ws.get(Workspace::SPEC_CAP, nb * 4);
        spec_caps_kernel<<<dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, c.stream>>>(h, nb, SS, cap, c.knobs.spec_tiny,
                                                                                        blo, bhi);
        HIP_CHECK(hipGetLastError());
        uint64_t *bstart = (uint64_t *)c.ws.get(Workspace::MSD_BSTART, (nb + 1) * 8);
        auto *cur = (unsigned long long *)c.ws.get(Workspace::SPEC_CUR, nb * 8);
        const uint64_t C = scan_counts_total(c, cap, nb, bstart, cur);  // (the cursors begin at the starts)
        if (spare && C * sizeof(Key<L>) > rq.spec_into_bytes) spare = nullptr;
        if (!spare) {  // the capacity is known now: both slack-sized buffers (one: fused rc merge, in place) must fit
            const uint64_t fr = c.ws.free_bytes();
            const double need = (double)C * KB * (rm || inplace ? 1.0 : 2.0);
            const double have = 0.9 * (double)fr + (double)c.ws.held_slot(Workspace::SPEC_A) +
                                (double)c.ws.held_slot(Workspace::SPEC_AC) +
                                (rm ? 0.0 : (double)c.ws.held_slot(Workspace::SPEC_B) +
                                                (double)c.ws.held_slot(Workspace::SPEC_BC));
            if (need > have) {
                if (c.knobs.debug) fprintf(stderr, "[mtg debug] speculative level: capacity %lu does not fit, exact level\n",
                                     (unsigned long)C);
                return ~0ull;
            }
        }
        Key<L> *sa = spare ? spare : (Key<L> *)c.ws.get(Workspace::SPEC_A, C * sizeof(Key<L>));
        uint32_t *sac = COUNTED ? (uint32_t *)c.ws.get(Workspace::SPEC_AC, C * 4) : nullptr;
        HIP_CHECK(hipMemsetAsync(&c.small->spec_ovf, 0, 4, c.stream));
        EventTimer tm(c.stream);
        tm.mark();
        msd_partition_kernel<L, COUNTED><<<dim3((unsigned)xcd_grid(tiles)), dim3(MSD_BLOCK), 0, c.stream>>>(
            *keys, sa, COUNTED ? *vals : nullptr, sac, npos, nbits, bb, bp, cur, 1,
            (const unsigned long long *)(bstart + 1), &c.small->spec_ovf, tv);
        HIP_CHECK(hipGetLastError());
        tm.mark();
        uint32_t povf = 0;
        HIP_CHECK(hipMemcpyAsync(&povf, &c.small->spec_ovf, 4, hipMemcpyDeviceToHost, c.stream));
        HIP_CHECK(hipStreamSynchronize(c.stream));
        if (rq.track_partition && c.build.radix_launches == 0) {
            c.build.radix_ms += tm.ms(0, 1);
            c.build.radix_launches += 1;
            c.build.radix_bytes += 2.0 * n * KB;
        }
        if (povf) {
            if (c.knobs.debug) fprintf(stderr, "[mtg debug] speculative level: a bucket overflowed, exact level\n");
            c.build.radix_ms = 0, c.build.radix_launches = 0, c.build.radix_bytes = 0;
            ++c.timings.spec_fallbacks;
            return ~0ull;
        }
        // g1: the padded input stays marked (pad) until this level succeeds -- a local pass that
        // overflows below returns ~0 and the caller's exact level must read the padded array again
        auto consumed_gap1 = [&]() {
            if (g1) pad = PaddedLayout{};  // the buckets below are compact per bucket
        };
        if (rm) {  // the fused rc merge over the speculative buckets
            uint32_t *cnt = (uint32_t *)c.ws.get(Workspace::SPEC_CAP, nb * 4);
            spec_counts_kernel<<<dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, c.stream>>>(bstart, cur, nb, cnt);
            HIP_CHECK(hipGetLastError());
            uint64_t *gbase = (uint64_t *)c.ws.get(Workspace::MSD_USTART, (nb + 1) * 8);
            scan_counts(c, cnt, nb, gbase);
            constexpr int CAP = MergeLocalTraits<L>::CAP;
            uint32_t *olist = (uint32_t *)c.ws.get(Workspace::MSD_OVF, nb * 4);  // the overflowing groups
            HIP_CHECK(hipMemsetAsync(&c.small->counter, 0, 4, c.stream));
            uint64_t *istart = rm->istart;
            // the canonical keys where they are: compact, or still in their own bucket layout (BuildState::gap,
            // whose compact index is cidx.start)
            const bool gapped = c.build.gap.valid && c.build.gap.dst == (const void *)rm->ck;
            const Key<L> *ck = gapped ? (const Key<L> *)c.build.gap.keys : rm->ck;
            const uint64_t *cgap = gapped ? c.build.gap.bstart : nullptr;
            // only the buckets either key set can occupy (a rank of a multi-GPU build owns ~1/P of them: the
            // other workgroups only wrote index entries, 0.8 ms a rank-step at P = 8); the index entries
            // outside them are 0 below and the merged count above
            uint64_t mlo = 0, mhi = nb;
            if (bp && !g1 && !gapped && rm->nc) {
                Key<L> e[4];
                HIP_CHECK(hipMemcpyAsync(&e[0], *keys, sizeof(Key<L>), hipMemcpyDeviceToHost, c.stream));
                HIP_CHECK(hipMemcpyAsync(&e[1], *keys + (n - 1), sizeof(Key<L>), hipMemcpyDeviceToHost, c.stream));
                HIP_CHECK(hipMemcpyAsync(&e[2], rm->ck, sizeof(Key<L>), hipMemcpyDeviceToHost, c.stream));
                HIP_CHECK(hipMemcpyAsync(&e[3], rm->ck + (rm->nc - 1), sizeof(Key<L>), hipMemcpyDeviceToHost, c.stream));
                HIP_CHECK(hipStreamSynchronize(c.stream));
                auto top = [&](const Key<L> &x) { return bits_at(shr(x, nbits - bp), 0, 32); };
                mlo = std::min(top(e[0]), top(e[2])) << (bb - bp);
                mhi = std::min<uint64_t>(nb, (std::max(top(e[1]), top(e[3])) + 1) << (bb - bp));
                if (istart && mlo < mhi) {
                    const uint64_t ilo = mlo << (rm->ib - bb), ihi = mhi << (rm->ib - bb), iend = 1ull << rm->ib;
                    if (ilo) fill_u64_kernel<<<dim3((unsigned)std::min<uint64_t>(ceil_div(ilo, 256), 4096)), dim3(256), 0,
                                               c.stream>>>(istart, 0, ilo, 0);
                    if (ihi < iend)
                        fill_u64_kernel<<<dim3((unsigned)std::min<uint64_t>(ceil_div(iend - ihi, 256), 4096)), dim3(256),
                                          0, c.stream>>>(istart, ihi, iend, n + rm->nc);
                    HIP_CHECK(hipGetLastError());
                } else if (mlo >= mhi) {
                    mlo = 0, mhi = nb;
                }
            }
            bucket_pieces(mlo, mhi, [&](uint64_t g0, unsigned cnt) {
                local_merge_kernel<L, COUNTED, CAP><<<dim3(cnt), dim3(512), 0, c.stream>>>(
                    sa, sac, bstart, nullptr, nullptr, ck, rm->cv, cidx.start, rm->out, rm->outc, olist,
                    &c.small->counter, bb, nbits, rm->ib, istart, cur, gbase, cgap, g0, c.knobs.merge_it);
                HIP_CHECK(hipGetLastError());
            });
            uint32_t novf = 0;
            HIP_CHECK(hipMemcpyAsync(&novf, &c.small->counter, 4, hipMemcpyDeviceToHost, c.stream));
            HIP_CHECK(hipStreamSynchronize(c.stream));
            if (novf) {  // the few big groups again with twice the LDS arrays, from the device-side list
                const uint32_t nlist = novf;
                HIP_CHECK(hipMemsetAsync(&c.small->counter, 0, 4, c.stream));
                bucket_pieces(0, nlist, [&](uint64_t g0, unsigned cnt) {
                    local_merge_kernel<L, COUNTED, 2 * CAP><<<dim3(cnt), dim3(512), 0, c.stream>>>(
                        sa, sac, bstart, nullptr, olist + g0, ck, rm->cv, cidx.start, rm->out, rm->outc, nullptr,
                        &c.small->counter, bb, nbits, rm->ib, istart, cur, gbase, cgap, 0, c.knobs.merge_it);
                    HIP_CHECK(hipGetLastError());
                });
                HIP_CHECK(hipMemcpyAsync(&novf, &c.small->counter, 4, hipMemcpyDeviceToHost, c.stream));
                HIP_CHECK(hipStreamSynchronize(c.stream));
            }
            if (novf) {
                if (c.knobs.debug) fprintf(stderr, "[mtg debug] speculative rc level: %u groups overflowed, exact level\n", novf);
                c.build.radix_ms = 0, c.build.radix_launches = 0, c.build.radix_bytes = 0;
                ++c.timings.spec_fallbacks;
                return ~0ull;
            }
            rm->done = true;
            consumed_gap1();
            ++c.timings.spec_levels;
            if (fine) ++c.timings.spec_fine_levels;
            if (gapped) c.build.gap.valid = false;  // merged: the canonical set is not needed compact
            if (istart) {  // index end = the merged count (a kernel argument: no host copy to wait for)
                const uint64_t R = n + rm->nc;
                set_u64_kernel<<<dim3(1), dim3(1), 0, c.stream>>>(istart + (1ull << rm->ib), R);
                HIP_CHECK(hipGetLastError());
                note_bucket_index(c, rm->out, R, istart, nbits - rm->ib);
            }
            if (c.knobs.debug)
                fprintf(stderr, "[mtg debug] speculative rc level: n=%lu capacity=%lu -> merged %lu\n", (unsigned long)n,
                        (unsigned long)C, (unsigned long)(n + rm->nc));
            return n;
        }
        // every bucket one group: [bstart[b], cur[b])
        Key<L> *sb = inplace ? sa : (Key<L> *)c.ws.get(Workspace::SPEC_B, C * sizeof(Key<L>));
        uint32_t *sbc = !COUNTED ? nullptr : inplace ? sac : (uint32_t *)c.ws.get(Workspace::SPEC_BC, C * 4);
        uint32_t *ucount = (uint32_t *)c.ws.get(Workspace::MSD_UCOUNT, (nb + 1) * 4);
        uint32_t *ovf = (uint32_t *)c.ws.get(Workspace::MSD_OVF, nb * 4);
        HIP_CHECK(hipMemsetAsync(ovf, 0, nb * 4, c.stream));
        HIP_CHECK(hipMemsetAsync(&c.small->counter, 0, 4, c.stream));
        const bool keycas = nbits < 64;
        constexpr int WPE = COUNTED ? 1 : MTG_LU_WPE;  // (the uncounted table fits 8 waves per SIMD at 64 VGPRs)
        // only the buckets the keys can occupy (blo, bhi above; a round of the batched collect fills a
        // fraction of them); the others count 0 keys
        HIP_CHECK(hipMemsetAsync(ucount, 0, (nb + 1) * 4, c.stream));
        bucket_pieces(blo, bhi, [&](uint64_t g0, unsigned cnt) {
            if (keycas && c.knobs.lu_fast)
                local_unique_kernel<1, COUNTED, true, 512, LocalTraits<1>::SLOTS / 2, false, WPE, true, false>
                    <<<dim3(cnt), dim3(512), 0, c.stream>>>(sa, sac, bstart, nullptr, nbits, bb, 0, sb, sbc, ucount, ovf,
                                                            &c.small->counter, cmax, cur, g0);
            else if (keycas)
                local_unique_kernel<1, COUNTED, true, 512, LocalTraits<1>::SLOTS / 2, false, WPE>
                    <<<dim3(cnt), dim3(512), 0, c.stream>>>(sa, sac, bstart, nullptr, nbits, bb, 0, sb, sbc, ucount, ovf,
                                                            &c.small->counter, cmax, cur, g0);
            else
                local_unique_kernel<1, COUNTED, false, 512, LocalTraits<1>::SLOTS / 2, false, 1>
                    <<<dim3(cnt), dim3(512), 0, c.stream>>>(sa, sac, bstart, nullptr, nbits, bb, 0, sb, sbc, ucount, ovf,
                                                            &c.small->counter, cmax, cur, g0);
            HIP_CHECK(hipGetLastError());
        });
        uint32_t novf = 0;
        HIP_CHECK(hipMemcpyAsync(&novf, &c.small->counter, 4, hipMemcpyDeviceToHost, c.stream));
        HIP_CHECK(hipStreamSynchronize(c.stream));
        if (c.knobs.spec_lu_fail) novf = 1;  // MTG_SPEC_LU_FAIL=1 (tests): as if a group had overflowed
        if (novf) {
            if (c.knobs.debug) fprintf(stderr, "[mtg debug] speculative level: %u groups overflowed, exact level\n", novf);
            c.build.radix_ms = 0, c.build.radix_launches = 0, c.build.radix_bytes = 0;
            ++c.timings.spec_fallbacks;
            return ~0ull;
        }
        uint64_t *ustart = (uint64_t *)c.ws.get(Workspace::MSD_USTART, (nb + 1) * 8);
        scan_counts(c, ucount, nb, ustart);
        if (!COUNTED && rq.defer_gather && c.knobs.defer_gather && rq.want_gidx) {
            // the fused rc merge follows: leave the distinct keys in their buckets (rq.gap); the
            // compact index of bucket g is ustart[g] (one bucket per group)
            uint64_t *gb = (uint64_t *)c.ws.get(Workspace::GAP_BSTART, (nb + 1) * 8);
            uint64_t *gu = (uint64_t *)c.ws.get(Workspace::GAP_USTART, (nb + 2) * 8);
            HIP_CHECK(hipMemcpyAsync(gb, bstart, (nb + 1) * 8, hipMemcpyDeviceToDevice, c.stream));
            HIP_CHECK(hipMemcpyAsync(gu, ustart, (nb + 1) * 8, hipMemcpyDeviceToDevice, c.stream));
            HIP_CHECK(hipMemcpyAsync(gu + nb + 1, ustart + nb, 8, hipMemcpyDeviceToDevice, c.stream));
            const uint64_t u = read_u64(c, (const unsigned long long *)(ustart + nb));
            rq.gap = GappedSet{true, sb, *keys, u, nb, gb, gu};
            consumed_gap1();
            ++c.timings.spec_levels;
            if (fine) ++c.timings.spec_fine_levels;
            rq.gidx = GroupIndex{*keys, u, bb, nbits, gu};
            if (c.knobs.debug)
                fprintf(stderr, "[mtg debug] speculative level: n=%lu capacity=%lu (%.2fx) -> %lu distinct, left in buckets\n",
                        (unsigned long)n, (unsigned long)C, (double)C / (double)n, (unsigned long)u);
            return u;
        }
        const bool index = rq.want_gidx;
        // a collect round's share of the whole set's index (rq.ridx), its buckets 2^(bits - bb) a group
        const bool rindex = !index && rq.ridx.start && bb <= rq.ridx.bits;
        uint64_t *gi = index ? (uint64_t *)c.ws.get(Workspace::CANON_IDX, (nb + 2) * 8) : rindex ? rq.ridx.start : nullptr;
        const unsigned ib = rindex ? rq.ridx.bits : bb;
        if (index || rindex) HIP_CHECK(hipMemsetAsync(&c.small->gidx_bad, 0, 4, c.stream));
        if (rq.out && (rq.out_cap == ~0ull || read_u64(c, (const unsigned long long *)(ustart + nb)) <= rq.out_cap)) {
            *keys = (Key<L> *)rq.out;  // (the caller's destination: the input is no longer read)
            if (COUNTED) *vals = rq.out_vals;
        }
        bucket_pieces(0, nb, [&](uint64_t g0, unsigned cnt) {
            group_gather_kernel<L, COUNTED><<<dim3(cnt), dim3(256), 0, c.stream>>>(
                sb, sbc, bstart, ustart, *keys, COUNTED ? *vals : nullptr, nullptr, nbits - ib, gi, &c.small->gidx_bad,
                g0, ib - bb, rindex ? rq.ridx.off : 0, rindex ? rq.ridx.lo : 0, rindex ? rq.ridx.hi : ~0ull);
            HIP_CHECK(hipGetLastError());
        });
        uint64_t u = 0;
        uint32_t ibad = 0;
        HIP_CHECK(hipMemcpyAsync(&u, ustart + nb, 8, hipMemcpyDeviceToHost, c.stream));
        if (index) {
            HIP_CHECK(hipMemcpyAsync(gi + nb, ustart + nb, 8, hipMemcpyDeviceToDevice, c.stream));
            HIP_CHECK(hipMemcpyAsync(gi + nb + 1, ustart + nb, 8, hipMemcpyDeviceToDevice, c.stream));
        }
        if (index || rindex) HIP_CHECK(hipMemcpyAsync(&ibad, &c.small->gidx_bad, 4, hipMemcpyDeviceToHost, c.stream));
        HIP_CHECK(hipStreamSynchronize(c.stream));
        if (index && !ibad) rq.gidx = GroupIndex{*keys, u, bb, nbits, gi};
        if (rindex) rq.ridx_written = !ibad;
        consumed_gap1();
        ++c.timings.spec_levels;
        if (fine) ++c.timings.spec_fine_levels;
        if (c.knobs.debug)
            fprintf(stderr, "[mtg debug] speculative level: n=%lu capacity=%lu (%.2fx) -> %lu distinct\n",
                    (unsigned long)n, (unsigned long)C, (double)C / (double)n, (unsigned long)u);
        return u;
    }
}

// The middle level of a 3-level sort without its exact histogram pass (a 60 GB read per configs[3]
// round): the level-2 buckets are sized from a sample with slack and rounded up to whole tiles of the
// level-3 tiling, the keys go from *keys into them in *alt (the caller's buffer of mid_bytes,
// SortRequest::spec_mid_into), and the padded result is described in *pad for level 3 as the speculative
// level-1 layout is for level 2 (tile t holds keys in its first tv[t] positions), with the
// level-2 prefix range of the keys (lo / hi) for level 3's bucket range.  False (nothing the
// caller needs touched) when it does not fit or a bucket overflowed: the exact level then.
template <int L, bool COUNTED>
static bool spec_mid_level(Ctx &c, Key<L> **keys, Key<L> **alt, uint64_t n, unsigned nbits, unsigned bp, unsigned bb,
                           uint64_t mid_bytes, PaddedLayout *pad) {
    if constexpr (L != 1 || COUNTED) {
        return false;
    } else {
        constexpr int TILE = MsdTraits<L>::TILE;
        constexpr uint32_t SS = 8;
        const uint64_t tiles = ceil_div(n, TILE);
        if (c.knobs.use_lsd || !c.knobs.spec_final || tiles < 64 * SS || bb - bp > 9 || bb > 24 || !bp) return false;
        const uint64_t nb = 1ull << bb;
        uint32_t *h = (uint32_t *)c.ws.get(Workspace::MSD_COUNTS, nb * 4);
        HIP_CHECK(hipMemsetAsync(h, 0, nb * 4, c.stream));
        // every 8th tile (level-1 buckets span hundreds of tiles here)
        msd_hist_kernel<L><<<dim3((unsigned)ceil_div(tiles, SS)), dim3(MSD_BLOCK), 0, c.stream>>>(*keys, n, nbits, bb, bp, h,
                                                                                                SS, 1, 1, nullptr);
        HIP_CHECK(hipGetLastError());
        Key<L> ends[2];
        HIP_CHECK(hipMemcpyAsync(&ends[0], *keys, sizeof(Key<L>), hipMemcpyDeviceToHost, c.stream));
        HIP_CHECK(hipMemcpyAsync(&ends[1], *keys + (n - 1), sizeof(Key<L>), hipMemcpyDeviceToHost, c.stream));
        HIP_CHECK(hipStreamSynchronize(c.stream));
        const uint64_t lo1 = ends[0].w[0] >> (nbits - bp), hi1 = ends[1].w[0] >> (nbits - bp);
        const uint64_t blo = lo1 << (bb - bp), bhi = std::min<uint64_t>(nb, (hi1 + 1) << (bb - bp));
        uint32_t *cap = (uint32_t *)c.ws.get(Workspace::SPEC_CAP, nb * 4);
        spec_caps_kernel<<<dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, c.stream>>>(h, nb, SS, cap, c.knobs.spec_tiny, blo,
                                                                                        bhi, (uint32_t)TILE);
        HIP_CHECK(hipGetLastError());
        uint64_t *bstart = (uint64_t *)c.ws.get(Workspace::MSD_BSTART, (nb + 1) * 8);
        const uint64_t C = scan_counts_total(c, cap, nb, bstart);
        if (C * sizeof(Key<L>) > mid_bytes) {
            if (c.knobs.debug) fprintf(stderr, "[mtg debug] speculative middle level: capacity %lu does not fit\n", (unsigned long)C);
            return false;
        }
        auto *cur = (unsigned long long *)c.ws.get(Workspace::SPEC_CUR, nb * 8);
        HIP_CHECK(hipMemcpyAsync(cur, bstart, nb * 8, hipMemcpyDeviceToDevice, c.stream));
        HIP_CHECK(hipMemsetAsync(&c.small->spec_ovf, 0, 4, c.stream));
        msd_partition_kernel<L, false><<<dim3((unsigned)xcd_grid(tiles)), dim3(MSD_BLOCK), 0, c.stream>>>(
            *keys, *alt, nullptr, nullptr, n, nbits, bb, bp, cur, 1, (const unsigned long long *)(bstart + 1),
            &c.small->spec_ovf, nullptr);
        HIP_CHECK(hipGetLastError());
        const uint64_t ntv = C / TILE;
        uint32_t *tv = (uint32_t *)c.ws.get(Workspace::SPEC_MID_TV, std::max<uint64_t>(ntv, 1) * 4);
        spec_tile_fill_kernel<<<dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, c.stream>>>(bstart, cur, nb, TILE, tv);
        HIP_CHECK(hipGetLastError());
        uint32_t povf = 0;
        HIP_CHECK(hipMemcpyAsync(&povf, &c.small->spec_ovf, 4, hipMemcpyDeviceToHost, c.stream));
        HIP_CHECK(hipStreamSynchronize(c.stream));
        if (povf) {
            if (c.knobs.debug) fprintf(stderr, "[mtg debug] speculative middle level: a bucket overflowed, exact level\n");
            ++c.timings.spec_fallbacks;
            return false;
        }
        std::swap(*keys, *alt);
        *pad = PaddedLayout{C, tv, blo, bhi};
        ++c.timings.spec_levels;
        if (c.knobs.debug)
            fprintf(stderr, "[mtg debug] speculative middle level: n=%lu capacity=%lu (%.2fx)\n", (unsigned long)n,
                    (unsigned long)C, (double)C / (double)n);
        return true;
    }
}

template <int L, bool COUNTED>
static uint64_t msd_sort_unique(Ctx &c, Key<L> **keys, Key<L> **alt, uint32_t **vals,
                                uint32_t **valt, uint64_t n, unsigned nbits, uint32_t cmax,
                                double dup, SortRequest<L> &rq) {
    const uint32_t *const hist1 = rq.hist1;
    const bool distinct = rq.distinct, level1_done = rq.level1_done;
    const std::vector<uint64_t> *const runs = rq.runs;
    RcMerge<L> *const rm = rq.rm;
    rq.ridx_written = false;
    rq.gidx = GroupIndex{};
    rq.gap = GappedSet{};
    if (n == 0) return 0;
    // the input while it is padded: the producer's level-1 layout until level 2 has read it, then a
    // speculative middle level's output until level 3 has
    PaddedLayout pad = level1_done ? rq.gap1 : PaddedLayout{};
    // *alt == nullptr (the single build after the speculative level-1 layout): the ping-pong buffer is taken
    // only by a path that needs it -- an exact level or the group passes -- never by the speculative level
    auto lazy_alt = [&]() {
        if (!*alt) *alt = (Key<L> *)c.ws.get(Workspace::KB, n * sizeof(Key<L>));
        if (COUNTED && !*valt) *valt = (uint32_t *)c.ws.get(Workspace::CB, n * 4);
    };
    constexpr uint32_t LIMIT = LocalTraits<L>::LIMIT;
    constexpr int TILE = MsdTraits<L>::TILE;
    const uint64_t tiles = ceil_div(n, TILE);
    // force_plan: the caller fixed the digits (the routed multi-GPU collect: level 1 is the routing digit)
    const MsdPlan plan = rq.force_plan ? *rq.force_plan : msd_plan<L>(c, n, nbits, dup);
    unsigned levels = plan.levels;
    unsigned digit_end[4] = {plan.digit_end[0], plan.digit_end[1], plan.digit_end[2], plan.digit_end[3]};
    unsigned b = 0;
    uint64_t *bstart = nullptr;
    uint64_t nbuckets = 1;
    auto run_level = [&](unsigned lev) {
        if (digit_end[lev] == 0) digit_end[lev] = std::min(nbits, digit_end[lev - 1] + 8);
        const unsigned bb = digit_end[lev], bp = digit_end[lev - 1];
        nbuckets = 1ull << bb;
        const uint32_t *cnt = hist1;
        // level 2 after a speculative level-1 layout reads the padded array (pad.n positions), and so
        // does level 3 after a speculative middle level (spec_mid_level)
        const bool g1 = pad.n && (lev == 2 ? level1_done : lev == 3);
        const uint64_t npos = g1 ? pad.n : n, ltiles = g1 ? ceil_div(npos, TILE) : tiles;
        const uint32_t *tv = g1 ? pad.tv : nullptr;
        if (lev != 1 || !hist1) {
            uint32_t *h = (uint32_t *)c.ws.get(Workspace::MSD_COUNTS, nbuckets * 4);
            HIP_CHECK(hipMemsetAsync(h, 0, nbuckets * 4, c.stream));
            if (bp == 0 && nbuckets <= 512) {
                const uint32_t nrows = (uint32_t)std::min<uint64_t>(tiles, 8192);
                uint32_t *rows = (uint32_t *)c.ws.get(Workspace::HIST_ROWS, (uint64_t)nrows * nbuckets * 4);
                msd_hist_rows_kernel<L><<<dim3(nrows), dim3(512), 0, c.stream>>>(*keys, n, nbits, bb, rows);
                HIP_CHECK(hipGetLastError());
                hist_rows_reduce_kernel<<<dim3(std::min<uint32_t>(nrows, 256), (unsigned)ceil_div(nbuckets, 256)),
                                          dim3(256), 0, c.stream>>>(rows, nrows, (uint32_t)nbuckets, h);
            } else {
                msd_hist_kernel<L><<<dim3((unsigned)ltiles), dim3(MSD_BLOCK), 0, c.stream>>>(*keys, npos, nbits, bb, bp,
                                                                                             h, 1, 1, 1, tv);
            }
            HIP_CHECK(hipGetLastError());
            cnt = h;
        }
        bstart = (uint64_t *)c.ws.get(Workspace::MSD_BSTART, (nbuckets + 1) * 8);
        scan_counts(c, cnt, nbuckets, bstart);
        if (lev == 1 && level1_done) {
            b = bb;
            return;
        }
        lazy_alt();  // (a partition level writes *alt)
        auto *cur = (unsigned long long *)c.ws.get(Workspace::MSD_CURSOR, nbuckets * 8);
        HIP_CHECK(hipMemcpyAsync(cur, bstart, nbuckets * 8, hipMemcpyDeviceToDevice, c.stream));
        EventTimer tm(c.stream);
        tm.mark();
        // 512-thread tiles (8 K keys, two workgroups per CU) on XCD-contiguous tiles: 3.77 ms for the
        // cfg2 level-2 pass vs 4.09 with 1024-thread tiles (16 K keys, one per CU) -- before the XCD
        // mapping the longer runs of the big tiles won (4.65 vs 5.3 ms); nontemporal access measured
        // the same (tools/part_bench.hip)
        msd_partition_kernel<L, COUNTED><<<dim3((unsigned)xcd_grid(ltiles)), dim3(MSD_BLOCK), 0, c.stream>>>(
            *keys, *alt, COUNTED ? *vals : nullptr, COUNTED ? *valt : nullptr, npos, nbits, bb, bp, cur, 1, nullptr,
            nullptr, tv);
        HIP_CHECK(hipGetLastError());
        if (g1) pad = PaddedLayout{};  // compact from here on
        tm.mark();
        if (rq.track_partition && c.build.radix_launches == 0) {  // first partition launch of the sort
            HIP_CHECK(hipStreamSynchronize(c.stream));
            c.build.radix_ms += tm.ms(0, 1);
            c.build.radix_launches += 1;
            c.build.radix_bytes += 2.0 * n * (sizeof(Key<L>) + (COUNTED ? 4 : 0));
        }
        std::swap(*keys, *alt);
        if (COUNTED) std::swap(*vals, *valt);
        b = bb;
    };
    if (runs && runs->size() >= 2 && runs->size() <= 129 && levels) {
        lazy_alt();
        // bucket layout of the top T bits straight from the runs' own order
        const unsigned T = digit_end[levels];
        const uint32_t P = (uint32_t)runs->size() - 1;
        nbuckets = 1ull << T;
        uint64_t *idx = (uint64_t *)c.ws.get(Workspace::RUN_IDX, (uint64_t)P * (nbuckets + 1) * 8);
        int64_t *delta = (int64_t *)c.ws.get(Workspace::RUN_DELTA, (uint64_t)P * nbuckets * 8);
        for (uint32_t j = 0; j < P; ++j) {
            const uint64_t r0 = (*runs)[j], rn = (*runs)[j + 1] - r0;
            bucket_index<L>(c, *keys + r0, rn, nbits - T, nbuckets, idx + (uint64_t)j * (nbuckets + 1));
        }
        bstart = (uint64_t *)c.ws.get(Workspace::MSD_BSTART, (nbuckets + 1) * 8);
        runs_delta_kernel<<<dim3((unsigned)std::min<uint64_t>(ceil_div(nbuckets + 1, 256), 16384)), dim3(256), 0,
                            c.stream>>>(idx, P, nbuckets, bstart, delta);
        HIP_CHECK(hipGetLastError());
        uint64_t *droff = (uint64_t *)c.ws.get(Workspace::RUN_OFF, (P + 1) * 8);
        HIP_CHECK(hipMemcpyAsync(droff, runs->data(), (P + 1) * 8, hipMemcpyHostToDevice, c.stream));
        runs_gather_kernel<L, COUNTED><<<dim3((unsigned)std::min<uint64_t>(ceil_div(n, 256), 65536)), dim3(256), 0,
                                         c.stream>>>(*keys, COUNTED ? *vals : nullptr, n, droff, P, delta,
                                                     nbuckets, nbits, T, *alt, COUNTED ? *valt : nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c.stream));  // `runs` is the caller's host vector
        std::swap(*keys, *alt);
        if (COUNTED) std::swap(*vals, *valt);
        b = T;
    } else {
        for (unsigned lev = 1; lev <= levels; ++lev) {
            // the last of 2 or 3 levels, the ones before it in place (3 levels: inputs over ~1.6e9 keys)
            // (any plain sort + unique too: configs[4]'s KMC records have no fused level 1)
            if (lev == levels && lev >= 2 && (lev == 2 || c.knobs.spec3) && (level1_done || (rm && distinct) || (!rm && !distinct))) {
                // the per-tile (fine) sample when the previous level's buckets span few tiles: 3 levels, or
                // a 10-bit level 1 on a small input (a tile-granular sample of ~30 tiles a bucket missed
                // by up to ~25 %)
                const bool fine = lev >= 3 || (n >> digit_end[lev - 1]) < 64ull * MsdTraits<L>::TILE;
                // the caller's spare buffer (rq.spec_into) once level 2 has moved the keys out of it
                Key<L> *spare = lev >= 3 && rq.spec_into && rq.spec_into != (void *)*keys ? (Key<L> *)rq.spec_into : nullptr;
                const uint64_t u = spec_final_level<L, COUNTED>(c, keys, vals, n, nbits, digit_end[lev - 1],
                                                                digit_end[lev], cmax, rq, pad, fine, spare);
                if (u != ~0ull) return u;
            }
            // a 3-level sort's middle level without its histogram pass, into the caller's buffer
            if (lev == 2 && levels == 3 && level1_done && !pad.n && c.knobs.spec_mid && c.knobs.spec3 && *alt &&
                rq.spec_mid_into == (void *)*alt &&
                spec_mid_level<L, COUNTED>(c, keys, alt, n, nbits, digit_end[1], digit_end[2], rq.spec_mid_bytes, &pad)) {
                b = digit_end[2];
                continue;
            }
            run_level(lev);
        }
    }

    lazy_alt();
    while (true) {
        // groups of consecutive buckets holding <= G keys; bigger buckets stand alone
        const uint64_t G = LIMIT / 4;
        uint64_t ngroups = 1;
        uint64_t *gstart;
        const uint64_t *gbucket_out = nullptr;
        if (b == 0) {
            gstart = (uint64_t *)c.ws.get(Workspace::MSD_GSTART, 16);
            set_pair_kernel<<<1, 1, 0, c.stream>>>(gstart, 0, n);
            HIP_CHECK(hipGetLastError());
        } else {
            uint32_t *gf = (uint32_t *)c.ws.get(Workspace::MSD_UCOUNT, (nbuckets + 1) * 4);
            const bool fuse = rm && distinct && b <= 32;
            uint64_t *cstart = nullptr;
            const uint64_t *gsize = bstart;
            if (fuse) {
                ensure_compact(c);  // this path reads the canonical keys compact
                // fused rc merge: the canonical keys of every bucket (bucket index of the sorted
                // set), and groups sized by rc + canonical keys together
                const GroupIndex &cidx = rm->cidx;
                if (cidx.keys == (const void *)rm->ck && cidx.n == rm->nc && cidx.bits == b && cidx.nbits == nbits) {
                    cstart = const_cast<uint64_t *>(cidx.start);  // the canonical sort's group starts
                } else {
                    cstart = (uint64_t *)c.ws.get(Workspace::RC_CSTART, (nbuckets + 2) * 8);
                    bucket_index<L>(c, rm->ck, rm->nc, nbits - b, nbuckets, cstart);
                }
                uint64_t *comb = (uint64_t *)c.ws.get(Workspace::RC_COMB, (nbuckets + 1) * 8);
                add_starts_kernel<<<dim3((unsigned)ceil_div(nbuckets + 1, 256)), dim3(256), 0, c.stream>>>(
                    bstart, cstart, nbuckets + 1, comb);
                HIP_CHECK(hipGetLastError());
                gsize = comb;
            }
            group_flags_kernel<<<dim3((unsigned)ceil_div(nbuckets, 256)), dim3(256), 0, c.stream>>>(
                gsize, nbuckets, G, gf);
            HIP_CHECK(hipGetLastError());
            uint64_t *gpos = (uint64_t *)c.ws.get(Workspace::MSD_USTART, (nbuckets + 1) * 8);
            ngroups = scan_counts_total(c, gf, nbuckets, gpos);
            gstart = (uint64_t *)c.ws.get(Workspace::MSD_GSTART, (ngroups + 1) * 8);
            // each group's bucket range: the fused rc merge's canonical ranges, or the output's bucket index
            uint64_t *gbucket = b <= 32 ? (uint64_t *)c.ws.get(Workspace::MSD_GBUCKET, (ngroups + 1) * 8) : nullptr;
            gbucket_out = gbucket;
            group_scatter_kernel<<<dim3((unsigned)ceil_div(nbuckets + 1, 256)), dim3(256), 0, c.stream>>>(
                bstart, gf, gpos, nbuckets, n, gstart, gbucket);
            HIP_CHECK(hipGetLastError());
            if (fuse && ngroups) {
                // sort the rc groups and merge them with the canonical keys in one pass
                constexpr int CAP = MergeLocalTraits<L>::CAP;
                uint32_t *olist = (uint32_t *)c.ws.get(Workspace::MSD_OVF, ngroups * 4);  // overflowing groups
                HIP_CHECK(hipMemsetAsync(&c.small->counter, 0, 4, c.stream));
                uint64_t *istart = rm->istart && rm->ib >= b ? rm->istart : nullptr;
                bucket_pieces(0, ngroups, [&](uint64_t g0, unsigned cnt) {
                    local_merge_kernel<L, COUNTED, CAP><<<dim3(cnt), dim3(512), 0, c.stream>>>(
                        *keys, COUNTED ? *vals : nullptr, gstart, gbucket, nullptr, rm->ck, rm->cv, cstart, rm->out,
                        rm->outc, olist, &c.small->counter, b, nbits, rm->ib, istart, nullptr, nullptr, nullptr, g0,
                        c.knobs.merge_it);
                    HIP_CHECK(hipGetLastError());
                });
                uint32_t novf = 0;
                HIP_CHECK(hipMemcpyAsync(&novf, &c.small->counter, 4, hipMemcpyDeviceToHost, c.stream));
                HIP_CHECK(hipStreamSynchronize(c.stream));
                if (novf) {  // the few big groups again with twice the LDS arrays, from the device-side list
                    const uint32_t nlist = novf;
                    HIP_CHECK(hipMemsetAsync(&c.small->counter, 0, 4, c.stream));
                    bucket_pieces(0, nlist, [&](uint64_t g0, unsigned cnt) {
                        local_merge_kernel<L, COUNTED, 2 * CAP><<<dim3(cnt), dim3(512), 0, c.stream>>>(
                            *keys, COUNTED ? *vals : nullptr, gstart, gbucket, olist + g0, rm->ck, rm->cv, cstart,
                            rm->out, rm->outc, nullptr, &c.small->counter, b, nbits, rm->ib, istart, nullptr, nullptr,
                            nullptr, 0, c.knobs.merge_it);
                        HIP_CHECK(hipGetLastError());
                    });
                    HIP_CHECK(hipMemcpyAsync(&novf, &c.small->counter, 4, hipMemcpyDeviceToHost, c.stream));
                    HIP_CHECK(hipStreamSynchronize(c.stream));
                    if (c.knobs.debug) fprintf(stderr, "[mtg debug] rc merge: %u big groups -> %u left\n", nlist, novf);
                }
                if (!novf) {
                    rm->done = true;
                    if (istart) {  // index end = the merged count (a kernel argument: no host copy to wait for)
                        const uint64_t R = n + rm->nc;
                        set_u64_kernel<<<dim3(1), dim3(1), 0, c.stream>>>(istart + (1ull << rm->ib), R);
                        HIP_CHECK(hipGetLastError());
                        note_bucket_index(c, rm->out, R, istart, nbits - rm->ib);
                    }
                    return n;  // the rc keys (distinct); rm->out holds U + n
                }
            }
        }
        uint32_t *ucount = (uint32_t *)c.ws.get(Workspace::MSD_UCOUNT, (ngroups + 1) * 4);
        uint32_t *ovf = (uint32_t *)c.ws.get(Workspace::MSD_OVF, ngroups * 4);
        HIP_CHECK(hipMemsetAsync(ovf, 0, ngroups * 4, c.stream));
        HIP_CHECK(hipMemsetAsync(&c.small->counter, 0, 4, c.stream));
        auto launch_local = [&](const uint32_t *glist, uint64_t count, unsigned sbits) {
            HIP_CHECK(hipMemsetAsync(&c.small->counter, 0, 4, c.stream));
            auto go = [&](auto keycas, auto sl, auto nodup) {
                constexpr bool KC = decltype(keycas)::value;
                constexpr int SL = decltype(sl)::value;
                constexpr bool ND = decltype(nodup)::value;
                constexpr int WPE = (L == 1 && KC && !ND && !COUNTED) ? MTG_LU_WPE : 1;
                bucket_pieces(0, count, [&](uint64_t g0, unsigned cnt) {
                    if constexpr (KC && !ND) {
                        if (c.knobs.lu_fast && sbits == 0) {  // the first launch: no key-range slices
                            local_unique_kernel<L, COUNTED, KC, 512, SL, ND, WPE, true, false><<<dim3(cnt), dim3(512), 0, c.stream>>>(
                                *keys, COUNTED ? *vals : nullptr, gstart, glist ? glist + g0 : nullptr, nbits, b, sbits,
                                *alt, COUNTED ? *valt : nullptr, ucount, ovf, &c.small->counter, cmax, nullptr,
                                glist ? 0 : g0);
                            return;
                        }
                        if (c.knobs.lu_fast) {
                            local_unique_kernel<L, COUNTED, KC, 512, SL, ND, WPE, true><<<dim3(cnt), dim3(512), 0, c.stream>>>(
                                *keys, COUNTED ? *vals : nullptr, gstart, glist ? glist + g0 : nullptr, nbits, b, sbits,
                                *alt, COUNTED ? *valt : nullptr, ucount, ovf, &c.small->counter, cmax, nullptr,
                                glist ? 0 : g0);
                            return;
                        }
                    }
                    // u128 keys (configs[2]): the state-word table at <= 80 VGPRs, so three workgroups fit a CU
                    // (the LDS allows three; 93 VGPRs allowed two)
                    if constexpr (L == 2 && !KC && !ND && !COUNTED) {
                        if (c.knobs.lu_wpe2) {
                            local_unique_kernel<L, COUNTED, KC, 512, SL, ND, 6><<<dim3(cnt), dim3(512), 0, c.stream>>>(
                                *keys, COUNTED ? *vals : nullptr, gstart, glist ? glist + g0 : nullptr, nbits, b, sbits,
                                *alt, COUNTED ? *valt : nullptr, ucount, ovf, &c.small->counter, cmax, nullptr,
                                glist ? 0 : g0);
                            return;
                        }
                    }
                    local_unique_kernel<L, COUNTED, KC, 512, SL, ND, WPE><<<dim3(cnt), dim3(512), 0, c.stream>>>(
                        *keys, COUNTED ? *vals : nullptr, gstart, glist ? glist + g0 : nullptr, nbits, b, sbits, *alt,
                        COUNTED ? *valt : nullptr, ucount, ovf, &c.small->counter, cmax, nullptr, glist ? 0 : g0);
                });
            };
            using T_ = std::true_type;
            using F_ = std::false_type;
            using SHalf = std::integral_constant<int, LocalTraits<L>::SLOTS / 2>;
            const bool keycas = L == 1 && nbits < 64;
            if (distinct) go(F_{}, SHalf{}, T_{});
            else if (keycas) go(T_{}, SHalf{}, F_{});
            else go(F_{}, SHalf{}, F_{});
            HIP_CHECK(hipGetLastError());
            uint32_t nov = 0;
            HIP_CHECK(hipMemcpyAsync(&nov, &c.small->counter, 4, hipMemcpyDeviceToHost, c.stream));
            HIP_CHECK(hipStreamSynchronize(c.stream));
            return nov;
        };
        uint32_t novf = launch_local(nullptr, ngroups, 0);
        if (c.knobs.trace)
            fprintf(stderr, "[mtg trace] msd n=%lu levels=%u b=%u groups=%lu overflow=%u\n", (unsigned long)n, levels, b,
                    (unsigned long)ngroups, novf);
        if (c.knobs.debug)
            fprintf(stderr, "[mtg debug] msd n=%lu nbits=%u levels=%u b=%u buckets=%lu groups=%lu overflow=%u\n",
                    (unsigned long)n, nbits, levels, b, (unsigned long)nbuckets, (unsigned long)ngroups, novf);
        // overflowing one-bucket groups: rerun them alone in 2, 4, 8, 16 key-range slices
        std::vector<uint32_t> flags;
        std::vector<uint64_t> gs;
        for (unsigned sbits = 1; novf && b && sbits <= 4 && b + sbits <= nbits; ++sbits) {
            flags.resize(ngroups);
            HIP_CHECK(hipMemcpyAsync(flags.data(), ovf, ngroups * 4, hipMemcpyDeviceToHost, c.stream));
            HIP_CHECK(hipStreamSynchronize(c.stream));
            std::vector<uint32_t> list;
            for (uint64_t g = 0; g < ngroups; ++g)
                if (flags[g]) list.push_back((uint32_t)g);
            uint32_t *dlist = (uint32_t *)c.ws.get(Workspace::MSD_GLIST, list.size() * 4);
            HIP_CHECK(hipMemcpyAsync(dlist, list.data(), list.size() * 4, hipMemcpyHostToDevice, c.stream));
            novf = launch_local(dlist, list.size(), sbits);  // syncs: `list` outlives the copy
            if (c.knobs.debug) fprintf(stderr, "[mtg debug]   sliced rerun sbits=%u groups=%zu -> overflow=%u\n", sbits, list.size(), novf);
        }
        if (novf) {
            flags.resize(ngroups);
            gs.resize(ngroups + 1);
            HIP_CHECK(hipMemcpyAsync(flags.data(), ovf, ngroups * 4, hipMemcpyDeviceToHost, c.stream));
            HIP_CHECK(hipMemcpyAsync(gs.data(), gstart, (ngroups + 1) * 8, hipMemcpyDeviceToHost, c.stream));
            HIP_CHECK(hipStreamSynchronize(c.stream));
            uint64_t ovf_keys = 0;
            for (uint64_t g = 0; g < ngroups; ++g)
                if (flags[g]) ovf_keys += gs[g + 1] - gs[g];
            if (c.knobs.debug) {
                fprintf(stderr, "[mtg debug]   fallback: %u groups, %lu keys\n", novf, (unsigned long)ovf_keys);
                int shown = 0;
                for (uint64_t g = 0; g < ngroups && shown < 5; ++g)
                    if (flags[g]) {
                        fprintf(stderr, "[mtg debug]     group %lu [%lu, %lu)\n", (unsigned long)g,
                                (unsigned long)gs[g], (unsigned long)gs[g + 1]);
                        ++shown;
                    }
            }
            if (ovf_keys * 20 > n && levels < 3 && digit_end[levels] < nbits) {
                run_level(++levels);  // many overflows: one more level for everything
                continue;
            }
            // the rest: LSD radix sort + unique of each group in place
            for (uint64_t g = 0; g < ngroups; ++g) {
                if (!flags[g]) continue;
                const uint64_t g0 = gs[g], m = gs[g + 1] - gs[g];
                Key<L> *fk = (Key<L> *)c.ws.get(Workspace::FB_K, m * sizeof(Key<L>));
                uint32_t *fv = COUNTED ? (uint32_t *)c.ws.get(Workspace::FB_V, m * 4) : nullptr;
                Key<L> *ka = *keys + g0, *kb = fk;
                uint32_t *va = COUNTED ? *vals + g0 : nullptr, *vb = fv;
                radix_sort<L, COUNTED>(c, &ka, &kb, &va, &vb, m, nbits, false);
                reset_small(c);
                const uint64_t ut = ceil_div(m, 2048);
                uint32_t ep;
                uint64_t *desc = acquire_desc(c, ut, &ep);
                unsigned long long *sums = nullptr;
                if (COUNTED) {
                    sums = (unsigned long long *)c.ws.get(Workspace::SUMS, m * 8);
                    HIP_CHECK(hipMemsetAsync(sums, 0, m * 8, c.stream));
                }
                unique_kernel<L, COUNTED><<<dim3((unsigned)ut), dim3(256), 0, c.stream>>>(
                    ka, va, m, *alt + g0, sums, desc, ep, &c.small->counter, &c.small->total, &c.small->error);
                HIP_CHECK(hipGetLastError());
                const uint64_t u = read_u64(c, &c.small->total);
                if (COUNTED)
                    count_clamp_kernel<<<dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(u, 256), 4096))),
                                         dim3(256), 0, c.stream>>>(sums, u, cmax, *valt + g0);
                const uint32_t u32 = (uint32_t)u;
                HIP_CHECK(hipMemcpyAsync(ucount + g, &u32, 4, hipMemcpyHostToDevice, c.stream));
                HIP_CHECK(hipStreamSynchronize(c.stream));
            }
        }
        // pack: ustart = exclusive scan of ucount, gather tmp (= *alt) -> *keys
        uint64_t *ustart = (uint64_t *)c.ws.get(Workspace::MSD_USTART, (ngroups + 1) * 8);
        scan_counts(c, ucount, ngroups, ustart);
        // the output's bucket index over the top b bits comes out of the gather (the fused rc merge
        // of the canonical keys reuses it instead of a bucket_index pass: 0.44 ms at configs[1])
        // (only for the sorts the fused rc merge follows: rq.want_gidx)
        const bool index = rq.want_gidx && gbucket_out && b > 0;
        uint64_t *gi = index ? (uint64_t *)c.ws.get(Workspace::CANON_IDX, (nbuckets + 2) * 8) : nullptr;
        if (index) HIP_CHECK(hipMemsetAsync(&c.small->gidx_bad, 0, 4, c.stream));
        if (rq.out &&
            (rq.out_cap == ~0ull || read_u64(c, (const unsigned long long *)(ustart + ngroups)) <= rq.out_cap)) {
            *keys = (Key<L> *)rq.out;  // (the caller's destination: the gather reads *alt only)
            if (COUNTED) *vals = rq.out_vals;
        }
        bucket_pieces(0, ngroups, [&](uint64_t g0, unsigned cnt) {
            group_gather_kernel<L, COUNTED><<<dim3(cnt), dim3(256), 0, c.stream>>>(
                *alt, COUNTED ? *valt : nullptr, gstart, ustart, *keys, COUNTED ? *vals : nullptr, gbucket_out,
                nbits - b, gi, &c.small->gidx_bad, g0);
            HIP_CHECK(hipGetLastError());
        });
        uint64_t u = 0;
        uint32_t ibad = 0;
        HIP_CHECK(hipMemcpyAsync(&u, ustart + ngroups, 8, hipMemcpyDeviceToHost, c.stream));
        if (index) {  // entries nbuckets, nbuckets + 1 = the key count
            HIP_CHECK(hipMemcpyAsync(gi + nbuckets, ustart + ngroups, 8, hipMemcpyDeviceToDevice, c.stream));
            HIP_CHECK(hipMemcpyAsync(gi + nbuckets + 1, ustart + ngroups, 8, hipMemcpyDeviceToDevice, c.stream));
            HIP_CHECK(hipMemcpyAsync(&ibad, &c.small->gidx_bad, 4, hipMemcpyDeviceToHost, c.stream));
        }
        HIP_CHECK(hipStreamSynchronize(c.stream));
        if (index && !ibad) rq.gidx = GroupIndex{*keys, u, b, nbits, gi};
        return u;
    }
}

template <int L>
static unsigned bucket_bits(uint64_t n, unsigned keybits) {
    // ~4 keys a bucket; at most 2^26 buckets up to 2^30 keys (configs[1]: 5.5 a bucket), 2^29 above: at
    // configs[3]'s share (4.7e9 real edges) 2^26 buckets held 69 edges each, and the dummy sink join's
    // staged class ranges (whole buckets at both ends) outgrew its LDS and fell back to global searches
    const unsigned cap = n > (1ull << 30) ? 29 : 26;
    unsigned b = 1;
    while (b < cap && (1ull << (b + 2)) < n) ++b;
    return std::min(b, keybits);
}

// MTG_DEBUG=1: host-side check that a device key array is strictly increasing
template <int L>
static void debug_check_sorted(Ctx &c, const char *what, const Key<L> *d, uint64_t n) {
    if (!c.knobs.debug || n == 0) return;
    std::vector<Key<L>> h(n);
    HIP_CHECK(hipMemcpyAsync(h.data(), d, n * sizeof(Key<L>), hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    uint64_t bad = 0;
    for (uint64_t i = 1; i < n; ++i) bad += !(h[i - 1] < h[i]);
    fprintf(stderr, "[mtg debug] %s: n=%lu, %lu order violations; first keys:", what,
            (unsigned long)n, (unsigned long)bad);
    for (uint64_t i = 0; i < std::min<uint64_t>(n, 8); ++i) fprintf(stderr, " %lx", (unsigned long)h[i].w[0]);
    fprintf(stderr, "\n");
}

// merge of two sorted arrays through the tiled merge-path kernels (boss_kernels.hpp)
template <int LO, int LA, bool LIFT, bool COUNTED, bool BCOUNTS>
static void merge_sorted(Ctx &c, const Key<LA> *a, const uint32_t *ac, uint64_t na,
                         const Key<LO> *b, const uint32_t *bc, uint64_t nb, unsigned K,
                         Key<LO> *out, uint32_t *oc, uint64_t off) {
    const uint64_t ntiles = ceil_div(na + nb, MergeTraits<LO>::TILE);
    if (!ntiles) return;
    uint64_t *splits = (uint64_t *)c.ws.get(Workspace::SPLITS, (ntiles + 1) * 8);
    merge_partition_kernel<LO, LA, LIFT><<<dim3((unsigned)ceil_div(ntiles + 1, 256)), dim3(256), 0, c.stream>>>(
        a, na, b, nb, K, ntiles, splits);
    HIP_CHECK(hipGetLastError());
    merge_kernel<LO, LA, LIFT, COUNTED, BCOUNTS><<<dim3((unsigned)ntiles), dim3(256), 0, c.stream>>>(
        a, ac, na, b, bc, nb, K, splits, out, oc, off);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mtg
