// ctx.hpp -- what every host stage of the construction path shares: the growable device workspace, the
// environment knobs, the state one build hands between its stages, and the small helpers over them.
// Included by boss_pipeline.hip only (after the kernel headers).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/mtg_boss.h"

namespace mtg {

#define HIP_CHECK(x)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess)                                                               \
            throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) +    \
                                     " at " #x);                                            \
    } while (0)

// growable device buffers, reused across builds
class Workspace {
  public:
    enum Slot {
        SEQ, STARTS, RCOUNTS, KA, KB, CA, CB, SUMS, DESC, HIST, STARTS_DIGIT, SMALL, BUCKETS,
        FLAGS, DA, DB, STREAM, SCOUNT, OW, OLAST, OWEIGHTS, MSD_COUNTS, MSD_BSTART,
        MSD_CURSOR, MSD_GSTART, MSD_UCOUNT, MSD_USTART, MSD_OVF, MSD_GLIST, FB_K, FB_V, RC_ALT, RC_ALTC, REAL, REALC, SPLITS, DTCNT, DTOFF, INFLAG, HIST1, HIST_ROWS,
        // multi-GPU build: exchange buffers, routing and the query join
        XA, XAC, XB, XBC, XHIST, XSTART_A, XSTART_B, XMAT, BOUNDS, RTCNT, RTOFF, XGATHER, QSEND, QRECV,
        QFLAG, QTCNT, QTOFF, DSRC, DSEND, DRECV, RUN_IDX, RUN_DELTA, RUN_OFF, KMC_LUT, KMC_REC, DUP_TABLE, FUSED_HIST, FUSED_CUR, STRIPE_CUR,
        LAST_BITS, DPOS, DWL, RANGE_BINS, MSD_GBUCKET, RC_CSTART, RC_COMB, RC_SENDC, PACKED, W4, FA_RAW, FA_TLAST, FA_PREV, FA_TA, FA_TB, FA_OA, FA_OB, FA_KOFF, RID_AT, BRUNS,
        SK_OWN, SK_TCNT, SK_TOFF, SK_WORDS, SK_LENS, SK_CNT, SK_RWORDS, SK_RLENS, SK_RCNT, SK_NW, SK_WOFF, SK_SEQ,
        SK_STARTS, SK_RID, CANON_IDX, SPEC_A, SPEC_B, SPEC_CAP, SPEC_CUR, GAP_BSTART, GAP_USTART, CANON, CANONC,
        FUSED_SEL, WN, SPEC_AC, SPEC_BC, SPEC1_CAPS, SPEC1_START, SPEC1_TV, QINDEX, DBITMAP, RC_L1START, RC_L1CUR, RC_TILEG,
        KA2, ROUND_DELTA, XA2, XAC2, CA2, SPEC_MID_TV,
        // counted FASTA input (kmer_counts.hpp): record starts, counts payload, windows and run offsets
        KC_RS, KC_CNT, KC_WCNT, KC_WOFF, KC_TCNT, KC_TOFF, NSLOTS
    };
    ~Workspace() {
        // every device block once, by its base (a slot or kept entry may be a piece of one: carve)
        for (auto &r : roots_)
            if (r.base) (void)hipFree(r.base);
    }
    void *get(Slot s, size_t bytes, size_t keep = 0, hipStream_t stream = nullptr) {
        Buf &b = bufs_[s];
        bytes = std::max<size_t>(bytes, 256);
        if (b.cap < bytes) {
            size_t cap = 0;
            int root = -1;
            void *p = take_cached(bytes, &cap, &root);
            if (!p) {
                cap = bytes + std::min<size_t>(bytes / 8, 1ull << 30);
                const auto t0 = std::chrono::steady_clock::now();
                bool dropped = false, carved = false;
                if (carve_always) {
                    p = take_cached(bytes, &cap, &root, true);
                    carved = p != nullptr;
                }
                if (!p && !try_malloc(&p, cap, &root)) {
                    // no room for a new block: a piece carved off a kept block that holds the request (the
                    // rest stays kept: the later stages of a batched build fit in the blocks its rounds gave
                    // back instead of each taking a whole one), and only then kept blocks freed one at a
                    // time, largest first (freeing kept blocks is what costs: ~12 ms per GB while the driver
                    // clears them, 2.3 s a build at configs[2] when every failed allocation dropped the
                    // whole cache).  MTG_WS_CARVE=1 (tests): carve before any new block
                    p = take_cached(bytes, &cap, &root, true);
                    carved = p != nullptr;
                    while (!p && !cache_.empty() && drop_largest()) {
                        dropped = true;
                        cap = bytes + std::min<size_t>(bytes / 8, 1ull << 30);
                        if (!try_malloc(&p, cap, &root)) p = nullptr;
                    }
                    if (!p && !try_malloc(&p, cap, &root)) {
                        size_t fr = 0, tot = 0;
                        (void)hipMemGetInfo(&fr, &tot);
                        throw std::runtime_error("HIP error out of memory: workspace slot " + std::to_string((int)s) +
                                                 " wants " + std::to_string(cap >> 20) + " MiB (held " +
                                                 std::to_string(held() >> 20) + " MiB in all slots, this one " +
                                                 std::to_string(b.cap >> 20) + " MiB; free " + std::to_string(fr >> 20) +
                                                 " MiB)");
                    }
                }
                if (carved) ++carves_;
                if (trace && cap >= (1ull << 28))
                    fprintf(stderr, "[mtg trace] workspace slot %d: %s %lu MiB%s, %.1f ms (held %lu MiB, kept %lu MiB)\n",
                            (int)s, carved ? "carved" : "new", (unsigned long)(cap >> 20),
                            dropped ? " after dropping the kept blocks" : "",
                            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                            (unsigned long)(held() >> 20), (unsigned long)(cached() >> 20));
            }
            if (keep && b.ptr) HIP_CHECK(hipMemcpyAsync(p, b.ptr, keep, hipMemcpyDeviceToDevice, stream));
            if (b.ptr) {
                HIP_CHECK(hipDeviceSynchronize());
                give_back(b);
            }
            b.ptr = p;
            b.cap = cap;
            b.root = root;
            ++gen_[s];
        }
        return b.ptr;
    }
    void swap(Slot a, Slot b) {
        std::swap(bufs_[a], bufs_[b]);
        ++gen_[a], ++gen_[b];
    }
    // the buffers a build's sort, rc, dummy and emit stages hold (not its input, look-back descriptors
    // or pass-A histograms): a build in rounds frees the previous build's before sizing its rounds
    void release_stage_buffers(bool keep_outputs = false) {
        // keep_outputs (mtg_boss_ctor_trim): the last build's device chunk arrays (W, last, weights) stay
        for (Slot sl : {KA, KB, CA, CB, SUMS, BUCKETS, FLAGS, DA, DB, STREAM, SCOUNT, OW, OLAST, OWEIGHTS, FB_K, FB_V,
                        RC_ALT, RC_ALTC, REAL, REALC, INFLAG, XA, XAC, XB, XBC, QSEND, QRECV, QFLAG, DSRC, DSEND,
                        DRECV, RC_SENDC, LAST_BITS, W4, WN, DPOS, DWL, CANON, CANONC, CANON_IDX, SPEC_A, SPEC_B,
                        SPEC_AC, SPEC_BC, KA2, XA2, XAC2, CA2})
            if (!keep_outputs || (sl != OW && sl != OLAST && sl != OWEIGHTS)) release(sl);
    }
    // a slot gives its buffer back (batched builds drop their round buffers before the later stages
    // grow).  The block is kept for the next get() of about its size rather than freed: freeing and
    // mapping again the ~200 GB of a configs[3] share cost seconds per build while the driver clears
    // the pages (and slowed the kernels running meanwhile).  A hipMalloc that fails frees the kept
    // blocks and tries again.
    void release(Slot s) {
        Buf &b = bufs_[s];
        if (b.ptr) {
            HIP_CHECK(hipDeviceSynchronize());
            give_back(b);
        }
        b.ptr = nullptr;
        b.cap = 0;
        b.root = -1;
        ++gen_[s];
    }
    // every byte the workspace holds, in slots and kept blocks
    uint64_t held() const {
        uint64_t t = cached();
        for (const auto &b : bufs_) t += b.cap;
        return t;
    }
    uint64_t cached() const {
        uint64_t t = 0;
        for (const auto &b : cache_) t += b.cap;
        return t;
    }
    // free HBM for new buffers: the device's free memory plus the kept blocks
    uint64_t free_bytes() const {
        size_t fr = 0, tot = 0;
        HIP_CHECK(hipMemGetInfo(&fr, &tot));
        return (uint64_t)fr + cached();
    }
    // the largest kept whole block freed (a block partly carved out to a slot stays); false: none
    bool drop_largest() {
        size_t big = cache_.size();
        for (size_t i = 0; i < cache_.size(); ++i)
            if (whole(cache_[i]) && (big == cache_.size() || cache_[i].cap > cache_[big].cap)) big = i;
        if (big == cache_.size()) return false;
        HIP_CHECK(hipDeviceSynchronize());
        free_root(cache_[big].root);
        cache_.erase(cache_.begin() + (long)big);
        return true;
    }
    void drop_cache() {
        if (cache_.empty()) return;
        HIP_CHECK(hipDeviceSynchronize());
        std::vector<Buf> keep;
        for (auto &b : cache_) {
            if (whole(b)) free_root(b.root);
            else keep.push_back(b);
        }
        cache_.swap(keep);
    }
    // end of a build: free the kept blocks no get() took during it (released in an earlier build and
    // idle since), so a big build's blocks do not pin HBM for the life of the constructor; the blocks
    // this build gave back stay for the next build of the same shape
    void end_build() {
        bool any = false;
        for (const auto &b : cache_) any |= b.age > 0 && whole(b);
        if (any) {
            HIP_CHECK(hipDeviceSynchronize());
            std::vector<Buf> keep;
            for (auto &b : cache_) {
                if (b.age > 0 && whole(b)) free_root(b.root);
                else keep.push_back(b);
            }
            cache_.swap(keep);
        }
        for (auto &b : cache_) b.age = 1;
    }
    uint64_t held_slot(Slot s) const { return bufs_[s].cap; }
    uint64_t carves() const { return carves_; }
    bool carve_always = false;  // MTG_WS_CARVE=1
    const void *peek(Slot s) const { return bufs_[s].ptr; }
    // bumped whenever the slot's buffer changes (regrown or released): a block given back may be
    // handed to another slot, so a pointer comparison alone cannot tell that the data is still there
    uint64_t generation(Slot s) const { return gen_[s]; }

  private:
    struct Buf {
        void *ptr = nullptr;
        size_t cap = 0;
        uint32_t age = 0;  // kept blocks: builds ended since it was given back (end_build)
        int root = -1;     // the device block (roots_) it is, or is a piece of
    };
    struct Root {
        void *base = nullptr;  // hipMalloc'ed, hipFree'd once when no piece of it is in use
        size_t cap = 0;
    };
    bool whole(const Buf &b) const { return b.root >= 0 && b.ptr == roots_[b.root].base && b.cap == roots_[b.root].cap; }
    bool try_malloc(void **p, size_t cap, int *root) {
        if (hipMalloc(p, cap) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        size_t i = 0;
        while (i < roots_.size() && roots_[i].base) ++i;
        if (i == roots_.size()) roots_.emplace_back();
        roots_[i] = Root{*p, cap};
        *root = (int)i;
        return true;
    }
    void free_root(int r) {
        (void)hipFree(roots_[r].base);
        roots_[r] = Root{};
    }
    // a slot's buffer back to the kept list, merged with the kept pieces of its block next to it (a
    // block whose pieces are all back is whole again: the next build of the same shape takes it whole)
    void give_back(Buf b) {
        b.age = 0;
        for (bool merged = true; merged;) {
            merged = false;
            for (size_t i = 0; i < cache_.size(); ++i) {
                Buf &o = cache_[i];
                if (o.root != b.root || b.root < 0) continue;
                if ((char *)o.ptr + o.cap == (char *)b.ptr) {
                    b.ptr = o.ptr, b.cap += o.cap;
                } else if ((char *)b.ptr + b.cap == (char *)o.ptr) {
                    b.cap += o.cap;
                } else {
                    continue;
                }
                cache_.erase(cache_.begin() + (long)i);
                merged = true;
                break;
            }
        }
        cache_.push_back(b);
    }
    // the smallest kept block of at least `bytes` and at most about twice that (a far bigger block
    // stays for the request it was made for); carve (the device has no room left): the smallest kept
    // block or piece that holds `bytes`, its front handed out and its rest kept when that is 256 MiB+
    void *take_cached(size_t bytes, size_t *cap, int *root, bool carve = false) {
        size_t best = cache_.size();
        for (size_t i = 0; i < cache_.size(); ++i)
            if (cache_[i].cap >= bytes && (carve || cache_[i].cap <= 2 * bytes + (64u << 20)) &&
                (best == cache_.size() || cache_[i].cap < cache_[best].cap))
                best = i;
        if (best == cache_.size()) return nullptr;
        Buf &k = cache_[best];
        void *p = k.ptr;
        *root = k.root;
        const size_t piece = (bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);  // 2 MiB aligned
        if (carve && k.cap >= piece + (256u << 20)) {
            *cap = piece;
            k.ptr = (char *)k.ptr + piece;
            k.cap -= piece;
            k.age = 0;
            return p;
        }
        *cap = k.cap;
        cache_.erase(cache_.begin() + (long)best);
        return p;
    }
    Buf bufs_[NSLOTS];
    uint64_t gen_[NSLOTS] = {};
    std::vector<Root> roots_;
    uint64_t carves_ = 0;

  public:
    bool trace = false;  // MTG_TRACE: report every fresh allocation of 256 MiB or more

  private:
    std::vector<Buf> cache_;
};

struct Small {  // one device word block, zeroed per use
    unsigned long long total;
    unsigned long long totals[2];
    unsigned long long fhist[8];
    uint32_t counter;
    uint32_t skip;
    uint32_t root_same;
    uint32_t bad_dummy;
    uint32_t bruns;  // bucket_index: listed long runs
    uint32_t fasta_bad;  // fasta_split_kernel: a '+' sequence line
    uint32_t gidx_bad;   // group_gather_kernel: the output bucket index was abandoned
    uint32_t spec_ovf;   // msd_partition_kernel: a speculative bucket overflowed
    uint32_t wbad;       // window_reads_kernel: the input is not one window per read
    unsigned long long wcursor;  // window_reads_kernel: keys written
    uint32_t kc_bad;     // kc_windows_kernel: a record shorter than k (1) or too long (2)
    uint32_t error;
};

class EventTimer {
  public:
    explicit EventTimer(hipStream_t s) : s_(s) {}
    ~EventTimer() {
        for (auto e : evs_) (void)hipEventDestroy(e);
    }
    int mark() {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        HIP_CHECK(hipEventRecord(e, s_));
        evs_.push_back(e);
        return (int)evs_.size() - 1;
    }
    double ms(int a, int b) {
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, evs_[a], evs_[b]));
        return t;
    }

  private:
    hipStream_t s_;
    std::vector<hipEvent_t> evs_;
};

// The few environment switches, read once per constructor (load_knobs) and constant after.  All but
// MTG_DEBUG / MTG_TRACE select alternate device paths that exist for correctness (fallbacks the parity
// tests force on small inputs), never a faster configuration.
struct Knobs {
    bool use_lsd = false;          // MTG_SORT=lsd: LSD onesweep + unique instead of MSD (the fallback
                                   // sort of overflowing groups, selectable for the parity tests)
    bool emit_slow = false;        // MTG_EMIT=slow: always the compacting emit kernel (the redundant-sink path)
    bool debug = false;            // MTG_DEBUG=1: host-side checks between stages
    bool trace = false;            // MTG_TRACE=1: per-step wall times and sizes of the dist build
    bool ws_carve = false;         // MTG_WS_CARVE=1: Workspace::carve_always
    bool fused = true;             // MTG_FUSED=0: K1 writes in window order, K2 partitions after
    uint64_t fused_min = 1ull << 22;  // MTG_FUSED_MIN: fewest window starts for the fused K1
    uint32_t force_ranges = 0;     // MTG_RANGES=P: collect in P key ranges (tests; else planned from memory)
    bool force_spill = false;      // MTG_SPILL=1: spill whenever the build runs in key ranges (tests)
    uint32_t hist_rows = 2048;     // MTG_HIST_ROWS: workgroups of the fused K1 histogram pass (tests
                                   // lower it so the grid-stride + prefetch loop runs on small inputs)
    uint64_t d2h_piece = 16ull << 20;  // MTG_D2H_PIECE=bytes: the piece of the packed W / narrowed weights copy to
                                   // the host (chunk_host.hpp), a multiple of 64 in [64, 1 Gi]
    bool d2h_piece_set = false;    // MTG_D2H_PIECE given: arrays of any size go in pieces, not only those of
                                   // 128 Mi rows / 16 Mi weights (tests run the piece loop on small inputs)
    bool fused_emit = true;        // MTG_FUSED_EMIT=0: K7 writes the lifted stream, K8 reads it (the
                                   // redundant-sink path)
    bool routed_min = false;       // MTG_ROUTED_CANON=min: the routed collect keeps min(fwd, rc)
    int dist_collect = 1;          // MTG_DIST_COLLECT: 1 routed keys (default), 0 super-k-mers
                                   // (=superkmer), 2 local collect + exchange of sorted runs (=local)
    unsigned fused_b1 = 0;         // MTG_FUSED_B1=n: the fused K1's level-1 digit forced to n bits (A/B runs)
    bool wide_b1 = true;           // MTG_WIDE_B1=0: no 10-bit level 1 (fused_plan)
    bool lu_fast = true;           // MTG_LU_FAST=0: local_unique_kernel's per-key list positions (A/B)
    bool fast2_ppt8 = true;        // MTG_FAST2_PPT8=0: the u128 packed-word pass B at 16 windows a thread (256 threads)
    bool rc_wide = true;           // MTG_RC_WIDE=0: the u128 rc sort planned like the unique (half-full merge groups)
    bool lu_wpe2 = true;           // MTG_LU_WPE2=0: the u128 local unique compiled for 1 wave per SIMD (no VGPR cap)
    bool fast2 = true;             // MTG_FAST2=0: the u128 rounds' pass B as the generic extract_partition_kernel
    uint32_t merge_it = 1;         // MTG_MERGE_IT: local_merge_kernel's least outputs per thread (A/B)
    bool range_scan = false;       // MTG_COLLECT=ranges: a build too big for one pass collects in key ranges
                                   // that re-scan the reads (both strands) even where the canonical
                                   // rounds of the fused K1 apply (collect_rounds_fused)
    bool kmc_mirror = true;        // add_kmc copies the first database to the device while reading it
    bool kspec = true;             // MTG_KSPEC=0: the fused K1 passes with K a runtime argument at K = 31 too
    bool dist_pull = true;         // MTG_DIST_SINKS=query: the multi-GPU sink join by routed queries
                                   // (target_split + query_join) instead of the pulled edge slices
    bool rc_fuse = true;           // MTG_RC_FUSE=0: the rc keys of a gapped canonical set written in canonical
                                   // order and partitioned by the rc sort's own level 1, not straight into
                                   // its level-1 buckets (rc_partition_gapped_kernel)
    int rc_spec = 1;               // MTG_RC_SPEC=0: those level-1 buckets sized by an exact histogram pass over the
                                   // whole canonical set, not from every 8th canonical bucket with slack (the
                                   // overflow fallback, forced); =tiny: half the estimate, rounded down to whole
                                   // tiles (tests force the overflow with it)
    bool dummy_bitmap = false;     // MTG_DUMMY_BITMAP=1: the source levels with few real chars as bits of a
                                   // bitmap (dummy_write_kernel) -- the sort gains 0.25 ms, the write pass
                                   // loses as much, so off by default
    bool dummy_ranks = true;       // MTG_DUMMY_SORT=lifted: sort the dummies as lifted keys, not as
                                   // dense u64 ranks (dummy_encode_kernel)
    bool round_index = true;        // MTG_ROUND_INDEX=0: the canonical set's index by a bucket_index pass
    bool defer_gather = true;       // MTG_DEFER_GATHER=0: the speculative level always gathers
    bool spec_rc = true;            // MTG_SPEC_RC=0: the rc sort's final level exact (tests the fallbacks)
    unsigned min_levels = 0;        // MTG_MSD_LEVELS=n: plan at least n MSD levels (tests the 3-level path)
    // MTG_SPEC3=0: the speculative final level only for 2-level plans.  (Sampled every 8th tile, the
    // level-3 buckets of level-2 buckets only a few tiles long were sized badly: at 20 M reads every
    // step overflowed into the exact level, sort 30.3 -> 38.9 ms; level 3 now samples every tile's
    // first eighth.)
    bool spec3 = true;
    // the speculative final level's local unique writes over its own buckets (each group is read whole
    // before it writes): one slack-sized buffer instead of two.  MTG_SPEC_INPLACE=0: two
    bool spec_inplace = true;
    // a collect round whose keys are sparse in the plan's final buckets (it spans more level-1 buckets
    // than its share: canonical k-mers crowd the small prefixes) takes one final bit fewer, so its local
    // unique runs fuller groups (configs[3]'s second round: 2.95 M groups of ~390 distinct keys, 25.7 vs
    // 20.6 ms for the first round's 1.25 M).  MTG_ROUND_BITS=0: the plan's bits in every round
    bool round_bits = true;
    bool rounds_one_b = true;  // two collect rounds share one pass B (collect_rounds_fused); MTG_ROUNDS_ONE_B=0: not
    // MTG_DIST_PIECES=n: the routed multi-GPU collect sends exchange 1 in n pieces on the exchange stream,
    // each sorted by its owner while the next one is in flight (routed_pieces); 1 = one exchange, then the sort
    uint32_t dist_pieces = 4;
    bool dist_pieces_set = false;  // MTG_DIST_PIECES given: exactly that many (else fewer for small shares)
    bool spec_final = true;  // MTG_SPEC=0: the exact final MSD level (histogram pass) instead of the
                             // sample-sized one (spec_final_level)
    bool spec_tiny = false;  // MTG_SPEC_CAPS=tiny: speculative buckets without slack (tests force the
                             // overflow fallback with it)
    bool spec_lu_fail = false;  // MTG_SPEC_LU_FAIL=1: the speculative level's local unique pass reports an
                                // overflow after it ran (tests the exact level after that late fallback)
    // MTG_SPEC_L1=0: the exact fused pass A (a histogram of every window) instead of the sampled one
    // and the speculative level-1 layout (fused_pass_b_spec), used from MTG_SPEC_L1_MIN windows on;
    // MTG_SPEC_L1_SAMPLE: pass A counts every n-th tile
    bool spec_l1 = true;
    bool spec_l1_tiny = false;  // MTG_SPEC_L1_CAPS=tiny: segments without slack (tests force its fallback)
    uint64_t spec_l1_min = 1ull << 28;
    uint32_t spec_l1_sample = 8;
    uint32_t spec_l1_stripes = 16;  // MTG_SPEC_L1_STRIPES: segments per level-1 bucket (a power of two <= 256)
    uint32_t spec_l1_slack = 16;    // MTG_SPEC_L1_SLACK: segment slack 1/n of the estimate (+ 3 sigma + 1024)
    bool spec_mid = true;  // MTG_SPEC_MID=0: a 3-level sort's middle level exact (spec_mid_level)
};

static Knobs load_knobs() {
    Knobs k;
    auto is = [](const char *name, const char *val) {
        const char *e = getenv(name);
        return e && std::string(e) == val;
    };
    k.use_lsd = is("MTG_SORT", "lsd");
    k.emit_slow = is("MTG_EMIT", "slow");
    k.fused = !is("MTG_FUSED", "0");
    k.fused_emit = !is("MTG_FUSED_EMIT", "0");
    k.dummy_ranks = !is("MTG_DUMMY_SORT", "lifted");
    k.range_scan = is("MTG_COLLECT", "ranges");
    k.wide_b1 = !is("MTG_WIDE_B1", "0");
    k.kmc_mirror = !is("MTG_KMC_MIRROR", "0");
    k.lu_fast = !is("MTG_LU_FAST", "0");
    k.lu_wpe2 = !is("MTG_LU_WPE2", "0");
    k.rc_wide = !is("MTG_RC_WIDE", "0");
    k.fast2_ppt8 = !is("MTG_FAST2_PPT8", "0");
    k.fast2 = !is("MTG_FAST2", "0");
    if (const char *e = getenv("MTG_MERGE_IT")) k.merge_it = (uint32_t)std::max(1L, std::min(64L, atol(e)));
    if (const char *v = getenv("MTG_FUSED_B1")) k.fused_b1 = (unsigned)std::min(10, std::max(0, atoi(v)));
    k.spec_final = !is("MTG_SPEC", "0");
    k.defer_gather = !is("MTG_DEFER_GATHER", "0");
    k.spec_rc = !is("MTG_SPEC_RC", "0");
    k.spec3 = !is("MTG_SPEC3", "0");
    k.rounds_one_b = !is("MTG_ROUNDS_ONE_B", "0");
    k.ws_carve = is("MTG_WS_CARVE", "1");
    k.spec_inplace = !is("MTG_SPEC_INPLACE", "0");
    k.round_bits = !is("MTG_ROUND_BITS", "0");
    k.round_index = !is("MTG_ROUND_INDEX", "0");
    k.spec_mid = !is("MTG_SPEC_MID", "0");
    if (const char *e = getenv("MTG_DIST_PIECES")) {
        k.dist_pieces = (uint32_t)std::max(1L, std::min(16L, atol(e)));
        k.dist_pieces_set = true;
    }
    k.spec_tiny = is("MTG_SPEC_CAPS", "tiny");
    k.spec_lu_fail = is("MTG_SPEC_LU_FAIL", "1");
    k.spec_l1 = !is("MTG_SPEC_L1", "0");
    k.dist_pull = !is("MTG_DIST_SINKS", "query");
    k.kspec = !is("MTG_KSPEC", "0");
    k.dummy_bitmap = is("MTG_DUMMY_BITMAP", "1");
    k.rc_fuse = !is("MTG_RC_FUSE", "0");
    k.rc_spec = is("MTG_RC_SPEC", "0") ? 0 : is("MTG_RC_SPEC", "tiny") ? 2 : 1;
    k.spec_l1_tiny = is("MTG_SPEC_L1_CAPS", "tiny");
    if (const char *e = getenv("MTG_SPEC_L1_STRIPES")) {
        const long v = atol(e);
        if (v >= 1 && v <= 256 && (v & (v - 1)) == 0) k.spec_l1_stripes = (uint32_t)v;
    }
    if (const char *e = getenv("MTG_SPEC_L1_SLACK")) k.spec_l1_slack = (uint32_t)std::max(2L, std::min(1024L, atol(e)));
    if (const char *e = getenv("MTG_SPEC_L1_MIN")) k.spec_l1_min = strtoull(e, nullptr, 10);
    if (const char *e = getenv("MTG_SPEC_L1_SAMPLE")) k.spec_l1_sample = (uint32_t)std::max(1L, std::min(64L, atol(e)));
    if (const char *v = getenv("MTG_MSD_LEVELS")) k.min_levels = (unsigned)std::min(3, std::max(0, atoi(v)));
    k.dist_collect = is("MTG_DIST_COLLECT", "superkmer") ? 0 : is("MTG_DIST_COLLECT", "local") ? 2 : 1;
    k.routed_min = is("MTG_ROUTED_CANON", "min");
    k.force_spill = is("MTG_SPILL", "1");
    k.debug = getenv("MTG_DEBUG") != nullptr;
    k.trace = getenv("MTG_TRACE") != nullptr;
    if (const char *e = getenv("MTG_FUSED_MIN")) k.fused_min = strtoull(e, nullptr, 10);
    if (const char *e = getenv("MTG_RANGES")) k.force_ranges = (uint32_t)std::max(0L, std::min(4096L, atol(e)));
    if (const char *e = getenv("MTG_HIST_ROWS")) k.hist_rows = (uint32_t)std::max(1L, std::min(2048L, atol(e)));
    if (const char *e = getenv("MTG_D2H_PIECE")) {
        k.d2h_piece = std::max<uint64_t>(64, std::min<uint64_t>(strtoull(e, nullptr, 10), 1ull << 30) & ~63ull);
        k.d2h_piece_set = true;
    }
    return k;
}

// what mtg_boss_ctor_create copies from its parameters: constant for the life of the constructor
struct Params {
    double mem_budget = 0;  // memory_preallocated (bytes; 0 = free HBM)
    bool disk = false;      // MTG_CONTAINER_VECTOR_DISK: the bounded-memory (range-batched) build
    std::string swap_dir;   // spill files of the disk container (swap_dir of initialize)
    uint64_t disk_cap = 0;  // at most this many bytes of spill files (disk_cap_bytes); the rest in RAM
};

// bucket index of a sorted distinct key set over its top `bits` bits (start[g] = the first key of bucket
// g, start[2^bits] and the entry after it = n): a sort's group starts when every group was one bucket
struct GroupIndex {
    const void *keys = nullptr;
    uint64_t n = 0;
    unsigned bits = 0, nbits = 0;
    const uint64_t *start = nullptr;
};

// a sorted distinct key set left in the speculative level's bucket layout (no group_gather_kernel):
// bucket g's keys at keys[bstart[g] ..), compact at ustart[g] .. (ustart[g + 1] - ustart[g] keys).
// rc_map and the fused rc merge read it there; ensure_compact() writes the compact array to dst when
// anything else needs it.
struct GappedSet {
    bool valid = false;
    const void *keys = nullptr;
    void *dst = nullptr;
    uint64_t u = 0, nb = 0;
    const uint64_t *bstart = nullptr, *ustart = nullptr;
};

// What one build hands between its own stages.  Nothing here outlives the build: dispatch_build resets
// it (reset_build_state) before every one.
struct BuildState {
    // the canonical set's bucket index over the rc sort's final bits (its own sort's, or
    // collect_rounds_fused's) and the set itself while it is still in buckets, from the collect until the
    // rc stage has merged it
    GroupIndex gidx;
    GappedSet gap;
    // bucket index over the real edges, built by the fused rc merge or the dummy stage and reused by the
    // split emit
    const void *bidx_keys = nullptr;
    uint64_t bidx_n = 0;
    const uint64_t *bidx = nullptr;
    unsigned bidx_shift = 0;
    uint64_t bidx_gen = 0;  // the BUCKETS slot's generation when the index was written
    // accumulated over the onesweep launches of the real-k-mer sorts
    double radix_ms = 0, radix_bytes = 0;
    uint64_t radix_launches = 0;
    double fused_ms = 0;  // device time of the last fused extract+partition launch
    bool host_output = false;  // the build's arrays go to the host (build_chunk): it may spill (want_spill)
};

struct Ctx {
    Ctx() {
        ws.carve_always = knobs.ws_carve;
        ws.trace = knobs.trace;
    }
    const Knobs knobs = load_knobs();
    Params params;
    Workspace ws;
    hipStream_t stream = nullptr;
    hipStream_t xstream = nullptr;  // the multi-GPU exchange stream (created by the first distributed build)
    Small *small = nullptr;
    mtg_boss_timings timings{};
    uint32_t epoch = 0;           // look-back granule epoch of the last launch
    size_t desc_words = 0;        // zeroed capacity of the descriptor buffer
    BuildState build;
};

static void reset_build_state(Ctx &c) { c.build = BuildState{}; }

static inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// zero the per-stage words; the error word is sticky for the whole build (checked at the end)
static void reset_small(Ctx &c) {
    HIP_CHECK(hipMemsetAsync(c.small, 0, offsetof(Small, error), c.stream));
}

static uint64_t read_u64(Ctx &c, const unsigned long long *p) {
    unsigned long long v = 0;
    HIP_CHECK(hipMemcpyAsync(&v, p, sizeof(v), hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    return v;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// MTG_TRACE: host wall time since the previous trace point (stream drained first)
struct Tracer {
    Ctx &c;
    int rank;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void operator()(const char *what, uint64_t a = 0, uint64_t b = 0) {
        if (!c.knobs.trace) return;
        HIP_CHECK(hipStreamSynchronize(c.stream));
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[mtg trace r%d] %-22s %9.3f ms  %lu %lu\n", rank, what,
                std::chrono::duration<double, std::milli>(now - t).count(), (unsigned long)a, (unsigned long)b);
        t = now;
    }
};

static void check_error_word(Ctx &c) {
    uint32_t e = 0;
    HIP_CHECK(hipMemcpyAsync(&e, &c.small->error, sizeof(e), hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    if (e & 1u) throw std::runtime_error("device look-back timed out (error word " + std::to_string(e) + ")");
    if (e) throw std::runtime_error("device partition counts disagree with the histogram pass (error word " +
                                    std::to_string(e) + ")");
}

// Descriptor array for one look-back launch plus its epoch.  Granules of older epochs read as
// "not ready", so the array is zeroed only when it grows or the 16-bit epoch wraps.
static uint64_t *acquire_desc(Ctx &c, uint64_t words, uint32_t *epoch) {
    uint64_t *d = (uint64_t *)c.ws.get(Workspace::DESC, words * 8);
    if (words > c.desc_words || c.epoch >= 0xFFFF) {
        size_t cap = std::max<size_t>(words, c.desc_words);
        d = (uint64_t *)c.ws.get(Workspace::DESC, cap * 8);
        HIP_CHECK(hipMemsetAsync(d, 0, cap * 8, c.stream));
        c.desc_words = cap;
        c.epoch = 0;
    }
    *epoch = ++c.epoch;
    return d;
}

// remember the bucket index over the real edges for the split emit's dummy ranks
static void note_bucket_index(Ctx &c, const void *keys, uint64_t n, const uint64_t *start, unsigned shift) {
    c.build.bidx_keys = keys;
    c.build.bidx_n = n;
    c.build.bidx = start;
    c.build.bidx_shift = shift;
    c.build.bidx_gen = c.ws.generation(Workspace::BUCKETS);
}

// the remembered bucket index still describes keys[0..n): the same array and count, and its entries still
// in the BUCKETS slot it was written to (a released or regrown slot may now hold another stage's data)
static bool bidx_valid(const Ctx &c, const void *keys, uint64_t n) {
    return c.build.bidx && c.build.bidx_keys == keys && c.build.bidx_n == n && (const void *)c.build.bidx == c.ws.peek(Workspace::BUCKETS) &&
           c.build.bidx_gen == c.ws.generation(Workspace::BUCKETS);
}

}  // namespace mtg
