// collect_stage.hpp -- the steps the bounded-memory collects share: the HBM budget, the key-range count
// pass and one range's extraction + local sort (kernels in range_extract.hpp), the growing sorted set the
// slices are appended to, and the owner's level-1 counts and sort request of the routed multi-GPU collect.
// None of them knows the exchange layer.  Included by boss_pipeline.hip only, after sort_unique.hpp.
#pragma once

#include "sort_unique.hpp"

namespace mtg {

struct BuildInput {
    const uint8_t *seq;
    uint64_t seq_len;
    const uint64_t *read_starts;
    const uint32_t *read_counts;
    uint64_t n_reads;
    const uint64_t *rid_at = nullptr;  // per-read counts: the read of every 4 K-position block
    int canon_mode = 1;                // the canonical representative the extraction keeps (cmode)
};

// the extraction kernels' canonical argument: 0 basic, 1 min(fwd, rc), 2 the strand whose top 12 bits hash
// smaller (boss_kernels.hpp: take_rc) -- any one representative per {x, rc x} gives the same real edges and
// weights; 2 spreads the representatives over the key space (the super-k-mer owners of a multi-GPU build)
static inline int cmode(const BuildInput &in, bool canonical) { return canonical ? in.canon_mode : 0; }

// window positions of the read buffer (valid or not)
static uint64_t n_windows(const BuildInput &in, unsigned K) { return in.seq_len >= K ? in.seq_len - K + 1 : 0; }

// the HBM budget a build plans its ranges or rounds with: memory_preallocated, else the free HBM (a
// rank's share of it: the `coresident` ranks on its GPU split it) plus what the workspace already holds
static double hbm_budget(const Ctx &c, uint32_t coresident = 1) {
    if (c.params.mem_budget > 0) return c.params.mem_budget;
    size_t fr = 0, tot = 0;
    HIP_CHECK(hipMemGetInfo(&fr, &tot));
    return 0.9 * ((double)fr / (double)std::max<uint32_t>(coresident, 1) + (double)c.ws.held());
}

// The count pass of a key-range collect: per-tile counts of the 4^RB_CHARS top-char bins (tbins) and
// their column sums (hist, on the device), both strands' k-mers when `both`.
template <int L2>
struct RangeScan {
    uint64_t tiles;
    uint16_t *tbins;
    unsigned long long *hist;
    uint32_t *tcnt = nullptr;  // a range's per-tile counts and their scan (tile_offsets)
    uint64_t *toff = nullptr;

    RangeScan(Ctx &c, const BuildInput &in, unsigned K, int both) {
        tiles = ceil_div(n_windows(in, K), RangeTraits<L2>::TILE);
        tbins = (uint16_t *)c.ws.get(Workspace::RANGE_BINS, std::max<uint64_t>(tiles, 1) * RB_BINS * 2);
        hist = (unsigned long long *)c.ws.get(Workspace::XHIST, RB_BINS * 8);
        HIP_CHECK(hipMemsetAsync(hist, 0, RB_BINS * 8, c.stream));
        if (!tiles) return;
        range_count_kernel<L2><<<dim3((unsigned)tiles), dim3(256), 0, c.stream>>>(in.seq, in.seq_len, K, both, tbins);
        HIP_CHECK(hipGetLastError());
        range_bins_reduce_kernel<<<dim3((unsigned)std::min<uint64_t>(tiles, 2048)), dim3(RB_BINS), 0, c.stream>>>(
            tbins, tiles, hist);
        HIP_CHECK(hipGetLastError());
    }
    // the device histogram as it stands -> *h; !sync: the caller synchronizes the stream before it reads *h
    void fetch(Ctx &c, std::vector<uint64_t> *h, bool sync = true) const {
        h->resize(RB_BINS);
        HIP_CHECK(hipMemcpyAsync(h->data(), hist, RB_BINS * 8, hipMemcpyDeviceToHost, c.stream));
        if (sync) HIP_CHECK(hipStreamSynchronize(c.stream));
    }
    void tile_offsets(Ctx &c) {
        tcnt = (uint32_t *)c.ws.get(Workspace::DTCNT, (tiles + 1) * 4);
        toff = (uint64_t *)c.ws.get(Workspace::DTOFF, (tiles + 1) * 8);
    }
};

// One range of a key-range collect: the nj k-mers of the bins `sel` (nj from the scan's histogram)
// extracted into KA (counts in CA), sorted and deduplicated; returns the distinct count, the keys in *ka
// (counts in *ca).  track: time the sort's first partition pass (the roofline's).
template <int L2, bool COUNTED>
static uint64_t extract_range_sorted(Ctx &c, const RangeScan<L2> &scan, const BuildInput &in, unsigned K, int both,
                                     uint32_t cmax, const BinSet &sel, uint64_t nj, bool track, Key<L2> **ka,
                                     Key<L2> **kb, uint32_t **ca, uint32_t **cb) {
    using K2 = Key<L2>;
    const uint64_t cap = std::max<uint64_t>(nj, 1);
    *ka = (K2 *)c.ws.get(Workspace::KA, cap * sizeof(K2));
    *kb = (K2 *)c.ws.get(Workspace::KB, cap * sizeof(K2));
    *ca = COUNTED ? (uint32_t *)c.ws.get(Workspace::CA, cap * 4) : nullptr;
    *cb = COUNTED ? (uint32_t *)c.ws.get(Workspace::CB, cap * 4) : nullptr;
    if (!nj) return 0;
    const uint64_t tiles = scan.tiles;
    range_tile_counts_kernel<<<dim3((unsigned)ceil_div(tiles, 4)), dim3(256), 0, c.stream>>>(scan.tbins, tiles, sel,
                                                                                             scan.tcnt);
    HIP_CHECK(hipGetLastError());
    scan_counts(c, scan.tcnt, tiles, scan.toff);
    range_write_kernel<L2, COUNTED><<<dim3((unsigned)tiles), dim3(256), 0, c.stream>>>(
        in.seq, in.seq_len, K, both, in.read_starts, in.read_counts, in.n_reads, in.rid_at, cmax, sel, scan.toff, *ka,
        *ca);
    HIP_CHECK(hipGetLastError());
    if (read_u64(c, (const unsigned long long *)(scan.toff + tiles)) != nj)
        throw std::runtime_error("range extraction count differs from its histogram");
    // the range fills sel.size() / RB_BINS of the top-char space: plan the MSD depth as if its keys
    // were spread over all of it
    const double spread = (double)RB_BINS / (double)std::max<uint32_t>(1, sel.size());
    const double dup = estimate_dup<L2>(c, *ka, nj, 8.0) / spread;
    SortRequest<L2> rq;
    rq.track_partition = track;
    return msd_sort_unique<L2, COUNTED>(c, ka, kb, ca, cb, nj, 2 * K, cmax, dup, rq);
}

// The sorted set a batched collect grows: every slice's distinct keys (and counts) appended in BOSS
// order to one slot pair, REAL / REALC or CANON / CANONC.
template <int L, bool COUNTED>
struct AppendSet {
    Ctx &c;
    Workspace::Slot kslot, vslot;
    Key<L> *keys = nullptr;
    uint32_t *vals = nullptr;
    uint64_t off = 0, cap = 0;  // keys appended; keys the slots hold

    // the set sized up front (a sort may then gather straight to tail())
    void reserve(uint64_t n) {
        cap = n;
        keys = (Key<L> *)c.ws.get(kslot, cap * sizeof(Key<L>));
        if (COUNTED) vals = (uint32_t *)c.ws.get(vslot, cap * 4);
    }
    Key<L> *tail() const { return keys + off; }
    uint32_t *tail_vals() const { return COUNTED ? vals + off : nullptr; }
    uint64_t room() const { return keys && (!COUNTED || vals) && off < cap ? cap - off : 0; }
    // U distinct keys at src (already at tail(): no copy).  The first fill sizes the set from the slice's
    // distinct ratio, U of its `den` keys, applied to the `num` keys of the whole set (+25 %); later
    // growth keeps what is already appended
    void append(const Key<L> *src, const uint32_t *srcc, uint64_t U, uint64_t num, uint64_t den) {
        if (off + U > cap) {
            const uint64_t want = off == 0 && den ? (uint64_t)((double)U / (double)den * (double)num * 1.25) + U
                                                  : (off + U) + (off + U) / 4;
            cap = std::max(want, off + U);
            keys = (Key<L> *)c.ws.get(kslot, cap * sizeof(Key<L>), off * sizeof(Key<L>), c.stream);
            if (COUNTED) vals = (uint32_t *)c.ws.get(vslot, cap * 4, off * 4, c.stream);
        }
        if (U && src != tail()) {
            HIP_CHECK(hipMemcpyAsync(tail(), src, U * sizeof(Key<L>), hipMemcpyDeviceToDevice, c.stream));
            if (COUNTED) HIP_CHECK(hipMemcpyAsync(tail_vals(), srcc, U * 4, hipMemcpyDeviceToDevice, c.stream));
        }
        off += U;
    }
    // the finished set (an empty one still has its slots); returns its size
    uint64_t finish(Key<L> **k, uint32_t **v) {
        if (!keys) {
            keys = (Key<L> *)c.ws.get(kslot, sizeof(Key<L>));
            if (COUNTED) vals = (uint32_t *)c.ws.get(vslot, 4);
        }
        *k = keys;
        *v = vals;
        return off;
    }
};

// The owner's sort of the routed multi-GPU collect: level 1 is the routing digit, B1 bits.  Its counts
// are the global pass-A histogram H (2^FUSED_HB bins) folded onto the owned level-1 buckets [rb0, rb1)
// -> hown (2^B1 entries); they must add up to the n keys the owner received.
static void owner_level1(const std::vector<uint64_t> &H, unsigned B1, uint64_t rb0, uint64_t rb1,
                         std::vector<uint32_t> &hown, uint64_t n, const char *differs) {
    hown.assign((size_t)1 << B1, 0);
    uint64_t nown = 0;
    for (uint32_t i = 0; i < (1u << FUSED_HB); ++i) {
        const uint32_t b = i >> (FUSED_HB - B1);
        if (b >= rb0 && b < rb1) {
            hown[b] += (uint32_t)H[i];
            nown += H[i];
        }
    }
    if (nown != n) throw std::runtime_error(differs);
}

// ... its plan: at least one partition pass after the routing digit
static MsdPlan owner_plan(const Ctx &c, uint64_t n, unsigned K, unsigned B1, double dup) {
    const MsdPlan plan = msd_plan<1>(c, n, 2 * K, dup);
    const unsigned T = plan.levels ? plan.digit_end[plan.levels] : 0;
    return level1_fixed_plan(B1, std::min(2 * K, std::max(T, B1 + 1)));
}

// ... and its request: the keys arrive scattered by level 1 (dh1: hown on the device), level 2 partitions
// the received runs in any order
static SortRequest<1> owner_request(const uint32_t *dh1, const MsdPlan *plan, bool track, bool gidx) {
    SortRequest<1> rq;
    rq.hist1 = dh1;
    rq.level1_done = true;
    rq.force_plan = plan;
    rq.track_partition = track;
    rq.want_gidx = gidx;
    return rq;
}

}  // namespace mtg
