// dummy_stage.hpp -- host drivers of the dummy-edge stage (K5/K6): the sort + unique of the raw dummy
// k-mers, the stage on one device, and the pieces the multi-GPU and the spilled builds share (kernels in
// boss_kernels.hpp and dist_kernels.hpp).  None of them knows the exchange layer.  Included by
// boss_pipeline.hip only, after sort_unique.hpp.
#pragma once

#include "sort_unique.hpp"

namespace mtg {

// the dense-rank dummy sort (boss_kernels.hpp: dummy_rank): `ranks` (u64 view of one of the two
// Draw-key buffers xa / xb) sorted + deduplicated, the distinct ranks decoded to lifted keys in
// whichever buffer does not hold them (both hold Draw lifted keys); returns D, *dk = the keys
template <int L3, int LR = 1>
static uint64_t sort_unique_dummy_ranks(Ctx &c, unsigned kb, Key<L3> *xa, Key<L3> *xb, Key<LR> *ranks, uint64_t Draw,
                                        Key<L3> **dk) {
    static_assert(sizeof(Key<LR>) <= sizeof(Key<L3>), "the rank buffers are the lifted key buffers");
    Key<LR> *ra = ranks, *rb = (void *)ranks == (void *)xa ? (Key<LR> *)xb : (Key<LR> *)xa;
    uint32_t *nv = nullptr;
    const unsigned nbits = dummy_rank_bits(kb);
    // (the real k-mers' MSD partition + LDS-hash unique on these ranks: dummy stage 4.4 -> 6.8 ms)
    radix_sort<LR, false>(c, &ra, &rb, &nv, &nv, Draw, nbits, false, true);  // (dense ranks: the low digit varies)
    reset_small(c);
    const uint64_t ut = ceil_div(Draw, 2048);
    uint32_t udesc_ep;
    uint64_t *udesc = acquire_desc(c, ut, &udesc_ep);
    unique_kernel<LR, false><<<dim3((unsigned)ut), dim3(256), 0, c.stream>>>(
        ra, nullptr, Draw, rb, nullptr, udesc, udesc_ep, &c.small->counter, &c.small->total, &c.small->error);
    HIP_CHECK(hipGetLastError());
    Key<L3> *outk = (void *)rb == (void *)xa ? xb : xa;
    // (a block per 256 dummies up to 16384 blocks, each a contiguous chunk; the grid is sized for Draw and the
    // kernel reads D from the device, so the copy of D to the host overlaps the decode)
    dummy_decode_kernel<L3, LR><<<dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(Draw, 256), 16384))),
                                  dim3(256), 0, c.stream>>>(rb, 0, kb, outk, &c.small->total);
    HIP_CHECK(hipGetLastError());
    const uint64_t D = read_u64(c, &c.small->total);
    *dk = outk;
    return D;
}

// sort + unique of the lifted dummy keys da[0..Draw) (db is the ping-pong buffer); returns D and
// leaves the distinct dummies in *dk.  For k <= 30 they are sorted as dense u64 ranks (8 LSD passes
// of 8-byte keys instead of 12 of 16-byte ones); otherwise, or when a key is not of the dummy shape,
// by an LSD sort of the lifted keys.  (An MSD sort of the dummies, planned for the 5-of-8 value
// density of lifted chars and with a read-before-CAS hash for their repeated keys, measured 24.5 vs
// 7.5 ms per cfg2 step and 24.9 vs 0.51 s per cfg3 step: groups of the $-padded source levels
// overflow the LDS tables and fall back.)
template <int L3>
static uint64_t sort_unique_dummies(Ctx &c, unsigned K, Key<L3> *da, Key<L3> *db, uint64_t Draw,
                                    Key<L3> **dk) {
    uint64_t D = 0;
    uint32_t *nv = nullptr;
    const unsigned kb = K - 1;
    const int LR = dummy_rank_limbs(kb);
    if (c.knobs.dummy_ranks && kb >= 1 && LR && (LR == 1 || L3 >= 2) && Draw) {
        HIP_CHECK(hipMemsetAsync(&c.small->bad_dummy, 0, 4, c.stream));
        const unsigned g = (unsigned)std::min<uint64_t>(ceil_div(Draw, 256), 16384);
        if (LR == 1)
            dummy_encode_kernel<L3, 1><<<dim3(g), dim3(256), 0, c.stream>>>(da, Draw, kb, (Key<1> *)db, &c.small->bad_dummy);
        else
            dummy_encode_kernel<L3, 2><<<dim3(g), dim3(256), 0, c.stream>>>(da, Draw, kb, (Key<2> *)db, &c.small->bad_dummy);
        HIP_CHECK(hipGetLastError());
        uint32_t bad = 0;
        HIP_CHECK(hipMemcpyAsync(&bad, &c.small->bad_dummy, 4, hipMemcpyDeviceToHost, c.stream));
        HIP_CHECK(hipStreamSynchronize(c.stream));
        if (!bad) {
            if (LR == 1) return sort_unique_dummy_ranks<L3, 1>(c, kb, da, db, (Key<1> *)db, Draw, dk);
            if constexpr (L3 >= 2) return sort_unique_dummy_ranks<L3, 2>(c, kb, da, db, (Key<2> *)db, Draw, dk);
        }
        if (c.knobs.debug) fprintf(stderr, "[mtg debug] dummy keys outside the rank shape: lifted sort\n");
    }
    {
        radix_sort<L3, false>(c, &da, &db, &nv, &nv, Draw, 3 * K, false);
        reset_small(c);
        const uint64_t ut = ceil_div(Draw, 2048);
        uint32_t udesc_ep;
        uint64_t *udesc = acquire_desc(c, ut, &udesc_ep);
        unique_kernel<L3, false><<<dim3((unsigned)ut), dim3(256), 0, c.stream>>>(
            da, nullptr, Draw, db, nullptr, udesc, udesc_ep, &c.small->counter, &c.small->total,
            &c.small->error);
        HIP_CHECK(hipGetLastError());
        D = read_u64(c, &c.small->total);
    }
    *dk = db;
    return D;
}

// the dummy keys dummy_write_kernel will write for the flagged edges (`levels` levels per source), counted
// per write tile and scanned: *toff = the tiles' offsets (the DTOFF slot), the total returned.
// (A DTCNT / DTOFF already larger stays as it is: Workspace::get only ever grows a slot.)
static uint64_t count_dummies(Ctx &c, const uint8_t *flags, const uint8_t *in_flag, uint64_t R, uint64_t wtiles,
                              unsigned levels, uint64_t **toff) {
    uint32_t *tcnt = (uint32_t *)c.ws.get(Workspace::DTCNT, (wtiles + 1) * 4);
    *toff = (uint64_t *)c.ws.get(Workspace::DTOFF, (wtiles + 1) * 8);
    if (!R) return 0;
    dummy_count_kernel<<<dim3((unsigned)wtiles), dim3(256), 0, c.stream>>>(flags, in_flag, R, levels, tcnt);
    HIP_CHECK(hipGetLastError());
    return scan_counts_total(c, tcnt, wtiles, *toff);
}

// K5/K6 on one device: dummy sinks and sources (all levels) of the sorted real edges ka[0..R)
template <int L2, int L3>
static uint64_t stage_dummies_local(Ctx &c, unsigned K, const Key<L2> *ka, uint64_t R, Key<L3> **dk) {
    using K3 = Key<L3>;
    const unsigned k = K - 1;
    const unsigned B = bucket_bits<L2>(R, 2 * K);
    const unsigned bshift = 2 * K - B;
    const uint64_t nb = 1ull << B;
    uint64_t *bstart = (uint64_t *)c.ws.get(Workspace::BUCKETS, (nb + 2) * 8);
    if (!(bidx_valid(c, ka, R) && c.build.bidx_shift == bshift && c.build.bidx == bstart)) {
        const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(R + 1, 256), 8192));
        bucket_index_kernel<L2><<<dim3((unsigned)g), dim3(256), 0, c.stream>>>(ka, R, bshift, nb, bstart);
        HIP_CHECK(hipGetLastError());
        note_bucket_index(c, ka, R, bstart, bshift);
    }
    uint8_t *flags = (uint8_t *)c.ws.get(Workspace::FLAGS, R + 1);
    uint8_t *in_flag = (uint8_t *)c.ws.get(Workspace::INFLAG, R + 1);
    const uint64_t wtiles = ceil_div(R, DummyTraits<L2>::WTILE);
    // the dense-rank path writes the source levels with <= DUMMY_BITMAP_M real chars as bits of a bitmap
    // (dummy_write_kernel), so the count pass counts kbig levels per source
    const bool bitmap_path = L2 == 1 && c.knobs.dummy_ranks && c.knobs.dummy_bitmap && k >= 1 && k <= 30;
    const unsigned ks = std::min<unsigned>(k, DUMMY_BITMAP_M + 1), kbig = bitmap_path ? k - ks : k;
    if (R) {
        HIP_CHECK(hipMemsetAsync(in_flag, 0, R, c.stream));
        dummy_sink_kernel<L2><<<dim3((unsigned)ceil_div(R, DummyTraits<L2>::TILE)), dim3(256), 0,
                                c.stream>>>(ka, R, K, bstart, bshift, flags, in_flag);
        HIP_CHECK(hipGetLastError());
    }
    uint64_t *toff;
    const uint64_t Draw = count_dummies(c, flags, in_flag, R, wtiles, kbig, &toff);
    *dk = nullptr;
    if constexpr (L2 == 1) {
        if (bitmap_path) {  // written as dense ranks: no lifted keys until the decode
            const uint64_t nbits = dummy_bitmap_base(ks), nwords = ceil_div(nbits, 32);
            uint32_t *bm = (uint32_t *)c.ws.get(Workspace::DBITMAP, nwords * 4);
            HIP_CHECK(hipMemsetAsync(bm, 0, nwords * 4, c.stream));
            const uint64_t cap = Draw + nbits;  // u64 ranks: the written ones, then at most every bit
            K3 *da = (K3 *)c.ws.get(Workspace::DA, cap * sizeof(K3));
            K3 *db = (K3 *)c.ws.get(Workspace::DB, cap * sizeof(K3));
            if (R) {
                dummy_write_kernel<L2, L3, true><<<dim3((unsigned)wtiles), dim3(256), 0, c.stream>>>(
                    ka, flags, in_flag, R, K, toff, da, kbig, bm);
                HIP_CHECK(hipGetLastError());
            }
            HIP_CHECK(hipMemcpyAsync(&c.small->total, &Draw, 8, hipMemcpyHostToDevice, c.stream));
            dummy_bitmap_ranks_kernel<<<dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(nwords, 256), 4096))),
                                        dim3(256), 0, c.stream>>>(bm, nwords, k, ks, (uint64_t *)da, &c.small->total);
            HIP_CHECK(hipGetLastError());
            const uint64_t Dall = read_u64(c, &c.small->total);  // (also orders the copy of the host local)
            if (c.knobs.debug)
                fprintf(stderr, "[mtg debug] dummies: %lu written + %lu from the bitmap (%u levels per source)\n",
                        (unsigned long)Draw, (unsigned long)(Dall - Draw), ks);
            if (!Dall) return 0;
            return sort_unique_dummy_ranks<L3>(c, k, da, db, (Key<1> *)da, Dall, dk);
        }
    }
    if (!Draw) return 0;
    K3 *da = (K3 *)c.ws.get(Workspace::DA, Draw * sizeof(K3));
    K3 *db = (K3 *)c.ws.get(Workspace::DB, Draw * sizeof(K3));
    if constexpr (L2 == 1) {
        if (c.knobs.dummy_ranks && k <= 30) {  // written as dense ranks: no lifted keys until the decode
            dummy_write_kernel<L2, L3, true><<<dim3((unsigned)wtiles), dim3(256), 0, c.stream>>>(ka, flags, in_flag,
                                                                                                  R, K, toff, da);
            HIP_CHECK(hipGetLastError());
            return sort_unique_dummy_ranks<L3>(c, k, da, db, (Key<1> *)da, Draw, dk);
        }
    }
    if constexpr (L2 <= 2 && L3 >= 2) {
        if (c.knobs.dummy_ranks && dummy_rank_limbs(k) == 2) {  // 30 < k <= 62: dense u128 ranks (configs[2]: k = 62)
            dummy_write_kernel<L2, L3, true, 2><<<dim3((unsigned)wtiles), dim3(256), 0, c.stream>>>(ka, flags, in_flag,
                                                                                                     R, K, toff, da);
            HIP_CHECK(hipGetLastError());
            return sort_unique_dummy_ranks<L3, 2>(c, k, da, db, (Key<2> *)da, Draw, dk);
        }
    }
    dummy_write_kernel<L2, L3><<<dim3((unsigned)wtiles), dim3(256), 0, c.stream>>>(ka, flags, in_flag, R, K,
                                                                                    toff, da);
    HIP_CHECK(hipGetLastError());
    return sort_unique_dummies<L3>(c, K, da, db, Draw, dk);
}

// ---- the pieces of the stage over a share of the edges (a rank's or a spilled range's): E[0..R) sorted

// bucket index of the real edges E[0..R) in the BUCKETS slot; `note` remembers it for the split emit's
// dummy ranks (note_bucket_index)
struct BucketIndex {
    uint64_t *bstart;
    unsigned bshift;
};
template <int L2>
static BucketIndex real_bucket_index(Ctx &c, const Key<L2> *E, uint64_t R, unsigned K, bool note) {
    const unsigned B = bucket_bits<L2>(R, 2 * K);
    const unsigned bshift = 2 * K - B;
    uint64_t *bstart = (uint64_t *)c.ws.get(Workspace::BUCKETS, ((1ull << B) + 2) * 8);
    bucket_index<L2>(c, E, R, bshift, 1ull << B, bstart);
    if (note) note_bucket_index(c, E, R, bstart, bshift);
    return {bstart, bshift};
}

// flags = first edge of its node, in_flag cleared: the state the query join starts from
template <int L2>
static void first_flags(Ctx &c, const Key<L2> *E, uint64_t R, uint8_t *flags, uint8_t *in_flag) {
    if (!R) return;
    HIP_CHECK(hipMemsetAsync(in_flag, 0, R, c.stream));
    first_flag_kernel<L2><<<dim3((unsigned)std::min<uint64_t>(ceil_div(R, 256), 16384)), dim3(256), 0, c.stream>>>(
        E, R, flags);
    HIP_CHECK(hipGetLastError());
}

// the dummy sources (`levels` levels each) of the edges no in-edge reaches, as the single build writes
// them: count -> scan -> write into the DSRC slot.  Returns the slot, *nsrc = the keys written.
template <int L2, int L3>
static Key<L3> *write_sources(Ctx &c, const Key<L2> *E, const uint8_t *flags, const uint8_t *in_flag, uint64_t R,
                              unsigned K, unsigned levels, uint64_t *nsrc) {
    using K3 = Key<L3>;
    const uint64_t wtiles = ceil_div(R, DummyTraits<L2>::WTILE);
    uint64_t *toff;
    const uint64_t n = count_dummies(c, flags, in_flag, R, wtiles, levels, &toff);
    K3 *src = (K3 *)c.ws.get(Workspace::DSRC, std::max<uint64_t>(n, 1) * sizeof(K3));
    if (n) {
        dummy_write_kernel<L2, L3><<<dim3((unsigned)wtiles), dim3(256), 0, c.stream>>>(E, flags, in_flag, R, K, toff,
                                                                                        src);
        HIP_CHECK(hipGetLastError());
    }
    *nsrc = n;
    return src;
}

// (defined with the exchange layer in boss_pipeline.hip)
__global__ void gather_strided_kernel(const uint64_t *__restrict__ src, uint64_t stride, uint32_t cnt,
                                      uint64_t *__restrict__ dst);

// the sink queries t = to_next(x, 0) of the edges as 4 sorted arrays in the QSEND slot (one per label of the
// querying edge, dist_kernels.hpp: target_split_kernel); every owner's share is a slice of each.  Returns
// the slot; with R > 0 also cstart[0..5) = the class starts and pos[cl * (P + 1) + j] = where owner j's
// slice of class cl starts (both absolute; column P is not the class end: the callers patch it)
template <int L2>
static Key<L2> *split_queries(Ctx &c, const Key<L2> *E, uint64_t R, unsigned K, uint32_t P,
                              const std::vector<uint64_t> &bounds, unsigned shift2, uint64_t *cstart, uint64_t *pos) {
    using K2 = Key<L2>;
    K2 *qs = (K2 *)c.ws.get(Workspace::QSEND, std::max<uint64_t>(R, 1) * sizeof(K2));
    if (!R) return qs;
    const uint64_t stiles = ceil_div(R, SplitTraits<L2>::TILE);
    uint32_t *tcnt = (uint32_t *)c.ws.get(Workspace::RTCNT, (4 * stiles + 1) * 4);
    uint64_t *toff = (uint64_t *)c.ws.get(Workspace::RTOFF, (4 * stiles + 1) * 8);
    target_split_kernel<L2, true><<<dim3((unsigned)stiles), dim3(256), 0, c.stream>>>(E, R, K, stiles, tcnt, nullptr,
                                                                                       nullptr);
    HIP_CHECK(hipGetLastError());
    scan_counts(c, tcnt, 4 * stiles, toff);
    target_split_kernel<L2, false><<<dim3((unsigned)stiles), dim3(256), 0, c.stream>>>(E, R, K, stiles, nullptr, toff,
                                                                                        qs);
    HIP_CHECK(hipGetLastError());
    uint64_t *g = (uint64_t *)c.ws.get(Workspace::XGATHER, (5 + 4 * (P + 1)) * 8);
    gather_strided_kernel<<<1, 256, 0, c.stream>>>(toff, stiles, 5, g);
    HIP_CHECK(hipGetLastError());
    uint64_t *db = (uint64_t *)c.ws.get(Workspace::BOUNDS, (P + 1) * 8);
    HIP_CHECK(hipMemcpyAsync(db, bounds.data(), (P + 1) * 8, hipMemcpyHostToDevice, c.stream));
    class_bounds_kernel<L2><<<dim3((unsigned)ceil_div(4 * (P + 1), 256)), dim3(256), 0, c.stream>>>(qs, g, db, P,
                                                                                                    shift2, g + 5);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(cstart, g, 5 * 8, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipMemcpyAsync(pos, g + 5, 4 * (P + 1) * 8, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));  // bounds / cstart / pos are host memory
    return qs;
}

// the received queries qr[0..nq) answered against the edges (query_join_kernel: in_flag of the edges hit,
// qflag of the queries), and the sinks of the missed ones counted and scanned; write_sinks writes them
// once the caller has sized their buffer
struct SinkJoin {
    uint64_t nsink = 0;
    uint8_t *qflag;
    uint64_t qtiles;
    uint32_t *qtcnt;
    uint64_t *qtoff;
};
template <int L2>
static SinkJoin answer_queries(Ctx &c, const Key<L2> *E, uint64_t R, const BucketIndex &bi, const Key<L2> *qr,
                               uint64_t nq, uint8_t *in_flag, Tracer *tr = nullptr) {
    SinkJoin j;
    j.qflag = (uint8_t *)c.ws.get(Workspace::QFLAG, nq + 1);
    if (nq) {
        query_join_kernel<L2><<<dim3((unsigned)ceil_div(nq, JoinTraits<L2>::TILE)), dim3(256), 0, c.stream>>>(
            E, R, bi.bstart, bi.bshift, qr, nq, in_flag, j.qflag);
        HIP_CHECK(hipGetLastError());
    }
    if (tr) (*tr)("answer q", nq);
    j.qtiles = ceil_div(nq, RT_TILE);
    j.qtcnt = (uint32_t *)c.ws.get(Workspace::QTCNT, (j.qtiles + 1) * 4);
    j.qtoff = (uint64_t *)c.ws.get(Workspace::QTOFF, (j.qtiles + 1) * 8);
    if (nq) {
        sink_count_kernel<<<dim3((unsigned)j.qtiles), dim3(RT_BLOCK), 0, c.stream>>>(j.qflag, nq, j.qtcnt);
        HIP_CHECK(hipGetLastError());
        j.nsink = scan_counts_total(c, j.qtcnt, j.qtiles, j.qtoff);
    }
    return j;
}

template <int L2, int L3>
static void write_sinks(Ctx &c, unsigned K, const Key<L2> *qr, uint64_t nq, const SinkJoin &j, Key<L3> *out) {
    sink_write_kernel<L2, L3><<<dim3((unsigned)j.qtiles), dim3(RT_BLOCK), 0, c.stream>>>(qr, j.qflag, nq, K, j.qtoff,
                                                                                        out);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mtg
