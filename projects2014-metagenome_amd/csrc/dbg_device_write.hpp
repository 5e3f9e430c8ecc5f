// dbg_device_write.hpp -- the graph files from a device chunk: the kernels of dbg_device.hpp compute the
// payload of dbg_io.hpp's write_dbg_payload, the host keeps the Huffman shape, the select supports,
// bit_vector_small and the framing.  Included by boss_pipeline.hip only, after its pipelines and ahead
// of the C ABI (it needs ctx.hpp, and chunk_host.hpp for pack_bits_kernel).
#pragma once

#include "chunk_host.hpp"
#include "ctx.hpp"
#include "dbg_device.hpp"
#include "dbg_io.hpp"
#include "dbg_prune.hpp"
#include "host_stage.hpp"

namespace mtg {
namespace {

struct DbgArgumentError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// device scratch of one call: hipMalloc'ed, regrown on demand, freed when the call returns
struct DevScratch {
    struct Buf {
        void *p = nullptr;
        uint64_t cap = 0;
    };
    std::vector<Buf *> all;
    ~DevScratch() {
        for (Buf *b : all) {
            if (b->p) (void)hipFree(b->p);  // waits for the device
            delete b;
        }
    }
    Buf *make() {
        all.push_back(new Buf());
        return all.back();
    }
    template <typename T>
    static T *ensure(Buf *b, uint64_t count) {
        const uint64_t bytes = std::max<uint64_t>(count * sizeof(T), 256);
        if (b->cap < bytes) {
            if (b->p) HIP_CHECK(hipFree(b->p));
            b->p = nullptr;
            b->cap = 0;
            HIP_CHECK(hipMalloc(&b->p, bytes));
            b->cap = bytes;
        }
        return (T *)b->p;
    }
    template <typename T>
    T *take(uint64_t count) { return ensure<T>(make(), count); }
};

struct PinnedBlocks {
    std::vector<void *> all;
    ~PinnedBlocks() {
        for (void *p : all) (void)PinnedPool::get().give(p);
    }
    template <typename T>
    T *take(uint64_t count) {
        all.push_back(PinnedPool::get().take(std::max<uint64_t>(count, 1) * sizeof(T)));
        return (T *)all.back();
    }
};

unsigned dbg_grid(uint64_t items) {
    const uint64_t g = ceil_div(std::max<uint64_t>(items, 1), dbgdev::kThreads);
    if (g > 0x7FFFFFFFull) throw std::runtime_error("write_dbg_device: too many rows for one launch");
    return (unsigned)g;
}

// the navigation directory over (W, packed last, n, F): d_nav / h_nav take 6 words (NF[0..4], then
// select_last(1)); one host synchronisation
dbgdev::Nav build_nav(DevScratch &dev, hipStream_t s, const uint8_t *W, const uint64_t *lastw, uint64_t n, uint64_t k,
                      const uint64_t *F, uint64_t *d_nav, uint64_t *h_nav) {
    using namespace dbgdev;
    const uint64_t nw = ceil_div(n, 64);
    uint32_t *cnt = dev.take<uint32_t>(6 * nw);
    uint64_t *sc = dev.take<uint64_t>(6 * nw + 1);
    uint64_t *dir = dev.take<uint64_t>(6 * (nw + 1));
    uint64_t *tmp = dev.take<uint64_t>(ceil_div(6 * nw, kScanTile) + 1);
    nav_count_kernel<<<dim3(dbg_grid(nw)), dim3(kThreads), 0, s>>>(W, lastw, n, nw, cnt);
    HIP_CHECK(hipGetLastError());
    exclusive_scan(cnt, 6 * nw, sc, tmp, s);
    nav_dir_kernel<<<dim3(dbg_grid(nw + 1), 6), dim3(kThreads), 0, s>>>(sc, nw, dir);
    HIP_CHECK(hipGetLastError());
    Nav nav{};
    nav.W = W;
    nav.last = lastw;
    nav.n = n;
    nav.k = k;
    nav.nw = nw;
    nav.last_rank = dir;
    for (int c = 0; c < 5; ++c) nav.wrank[c] = dir + (uint64_t)(1 + c) * (nw + 1);
    FVec f{};
    for (int c = 0; c < 5; ++c) f.F[c] = F[c];
    nav_nf_kernel<<<dim3(1), dim3(64), 0, s>>>(nav, f, d_nav);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_nav, d_nav, 6 * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int c = 0; c < 5; ++c) nav.NF[c] = h_nav[c];
    return nav;
}

// The level-synchronous walk of the source-dummy tree (mark_all_dummy_edges): walked[i] (n zeroed bytes) = 1
// for every row of a node that holds a '$'.  d_root: select_last(1) on the device (build_nav's sixth word);
// h_count: one pinned word.  One host synchronisation per level; needs n > 1.
void walk_source_dummies(DevScratch &dev, hipStream_t s, const dbgdev::Nav &nav, const uint64_t *d_root,
                         uint64_t *h_count, uint8_t *walked, const char *who) {
    using namespace dbgdev;
    const uint64_t n = nav.n, k = nav.k;
    DevScratch::Buf *fb[2] = {dev.make(), dev.make()}, *cb = dev.make(), *sb = dev.make(), *tb = dev.make();
    uint64_t *cur = DevScratch::ensure<uint64_t>(fb[0], 1);
    HIP_CHECK(hipMemcpyAsync(cur, d_root, 8, hipMemcpyDeviceToDevice, s));
    uint64_t m = 1;
    for (uint64_t depth = 0; depth < k && m; ++depth) {
        const bool expand = depth + 1 < k;
        uint32_t *cnt = DevScratch::ensure<uint32_t>(cb, m);
        mask_count_kernel<<<dim3(dbg_grid(m)), dim3(kThreads), 0, s>>>(nav, cur, m, expand ? 1 : 0, cnt, walked);
        HIP_CHECK(hipGetLastError());
        if (!expand) break;
        uint64_t *sc = DevScratch::ensure<uint64_t>(sb, m + 1);
        exclusive_scan(cnt, m, sc, DevScratch::ensure<uint64_t>(tb, ceil_div(m, kScanTile) + 1), s);
        HIP_CHECK(hipMemcpyAsync(h_count, sc + m, 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const uint64_t next_m = *h_count;
        if (next_m > n)
            throw DbgArgumentError(std::string(who) + ": the arrays are no BOSS table (the source-dummy tree outgrows the rows)");
        if (!next_m) break;
        uint64_t *next = DevScratch::ensure<uint64_t>(fb[(depth + 1) & 1], next_m);
        mask_expand_kernel<<<dim3(dbg_grid(m)), dim3(kThreads), 0, s>>>(nav, cur, m, sc, next, next_m);
        HIP_CHECK(hipGetLastError());
        cur = next;
        m = next_m;
    }
}

// The files from any device (W, last, n, F).  `flagged` (may be null): the mask's source-dummy flags, one
// byte per row, already computed (the pruned path); without it mask_dummy walks the source-dummy tree
// here.  pre_device_ms: device time the caller spent before this call, added to the timings.
uint64_t write_dbg_device_stages(Ctx &ctx, const mtg_boss_device_chunk &ch, unsigned bits_per_count,
                                 const std::string &base, uint64_t mode, int mask_dummy, int64_t suffix_length,
                                 mtg_dbg_write_timings *T, const uint8_t *flagged_in, double pre_device_ms) {
    using namespace dbgdev;
    hipStream_t s = ctx.stream;
    const uint64_t n = ch.n, nw = ceil_div(n, 64), k = ch.k;
    const uint64_t L = dbgio::indexed_suffix_length(suffix_length, k);
    if (L > 13) throw std::runtime_error("write_dbg_device: a suffix index of 4^" + std::to_string(L) +
                                         " ranges does not fit the device writer");
    const bool navigate = (mask_dummy && !flagged_in) || L;
    const bool weighted = ch.weights && bits_per_count;
    PinnedBlocks pin;  // given back after the device scratch is freed (hipFree waits for the copies)
    DevScratch dev;
    hipEvent_t ev[2];
    for (auto &e : ev) HIP_CHECK(hipEventCreate(&e));
    struct EvGuard {
        hipEvent_t *ev;
        ~EvGuard() {
            for (int i = 0; i < 2; ++i) (void)hipEventDestroy(ev[i]);
        }
    } ev_guard{ev};
    HIP_CHECK(hipEventRecord(ev[0], s));

    enum { S_HIST = 0, S_NAV = 18, S_NVALID = 24, S_ONES = 25, S_COUNT = 26, S_WORDS = 32 };
    uint64_t *d_small = dev.take<uint64_t>(S_WORDS);
    uint64_t *h_small = pin.take<uint64_t>(S_WORDS);
    HIP_CHECK(hipMemsetAsync(d_small, 0, S_WORDS * 8, s));

    // 1. W histogram per tile, its scan, the shape (host)
    const uint64_t ntiles = ceil_div(n, kTile), nh = 17 * ntiles;
    if (ntiles > 0x7FFFFFFFull) throw std::runtime_error("write_dbg_device: too many rows for one launch");
    uint32_t *hist = dev.take<uint32_t>(nh);
    uint64_t *hscan = dev.take<uint64_t>(nh + 1);
    DevScratch::Buf *scan_tmp_buf = dev.make();
    auto scan_tmp = [&](uint64_t items) { return DevScratch::ensure<uint64_t>(scan_tmp_buf, ceil_div(items, kScanTile) + 1); };
    w_hist_kernel<<<dim3((unsigned)ntiles), dim3(kThreads), 0, s>>>(ch.W, n, ntiles, hist);
    HIP_CHECK(hipGetLastError());
    exclusive_scan(hist, nh, hscan, scan_tmp(nh), s);
    {
        GatherIdx g{};
        for (int i = 0; i < 18; ++i) g.idx[i] = (uint64_t)i * ntiles;
        gather_kernel<<<dim3(1), dim3(64), 0, s>>>(hscan, g, 18, d_small + S_HIST);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipMemcpyAsync(h_small, d_small, 18 * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h_small[17] != h_small[16])
        throw DbgArgumentError("write_dbg_device: W holds " + std::to_string(h_small[17] - h_small[16]) +
                               " values above 15 (a BOSS label is a 4-bit code)");
    dbgio::DbgPayload P;
    P.n = n;
    P.L = L;
    sdslio::WtHuffPayload &wt = P.wt;
    uint64_t freq[256] = {0};
    WtTable tb{};
    for (int c = 0; c < 16; ++c) {
        freq[c] = h_small[c + 1] - h_small[c];
        tb.row_base[c] = h_small[c];
        wt.sigma += freq[c] != 0;
    }
    wt.n = n;
    wt.tree = sdslio::huff_shape(freq);
    wt.total = sdslio::huff_total_bits(wt.tree);
    std::vector<int> inner_of(wt.tree.nodes.size(), -1);
    for (size_t v = 0; v < wt.tree.nodes.size(); ++v)
        if (wt.tree.nodes[v].child[0] != 0xFFFF) {
            if (tb.ninner >= (uint32_t)kMaxInner) throw std::runtime_error("write_dbg_device: bad Huffman shape");
            inner_of[v] = (int)tb.ninner;
            tb.bv_pos[tb.ninner++] = wt.tree.nodes[v].bv_pos;
        }
    for (int c = 0; c < 16; ++c) {
        if (wt.tree.leaf[c] == 0xFFFF) continue;
        const uint64_t path = wt.tree.path[c], len = path >> 56;
        uint16_t v = 0;
        for (uint64_t d = 0; d < len; ++d) {
            const uint64_t b = (path >> d) & 1;
            tb.under[inner_of[v]] |= (uint16_t)(1u << c);
            if (b) tb.one[inner_of[v]] |= (uint16_t)(1u << c);
            v = wt.tree.nodes[v].child[b];
        }
    }

    // 2. the node bits; 4. their rank_support_v<1> words
    const uint64_t bvw = ceil_div(wt.total, 64);
    uint64_t *bv = dev.take<uint64_t>(bvw);
    HIP_CHECK(hipMemsetAsync(bv, 0, std::max<uint64_t>(bvw, 1) * 8, s));
    if (tb.ninner) {
        wt_fill_kernel<<<dim3((unsigned)ntiles), dim3(kThreads), 0, s>>>(ch.W, n, ntiles, hscan, tb, bv, bvw);
        HIP_CHECK(hipGetLastError());
    }
    const uint64_t nb_v = (bvw >> 3) + 1;
    uint64_t *rank_v = dev.take<uint64_t>(2 * nb_v);
    {
        uint32_t *cnt = dev.take<uint32_t>(nb_v);
        uint64_t *sc = dev.take<uint64_t>(nb_v + 1);
        rank_blocks_kernel<8><<<dim3(dbg_grid(nb_v)), dim3(kThreads), 0, s>>>(bv, bvw, nb_v, cnt, rank_v);
        HIP_CHECK(hipGetLastError());
        exclusive_scan(cnt, nb_v, sc, scan_tmp(nb_v), s);
        rank_first_kernel<<<dim3(dbg_grid(nb_v)), dim3(kThreads), 0, s>>>(sc, nb_v, rank_v);
        HIP_CHECK(hipGetLastError());
    }

    // 3. last packed; 4. its rank_support_v5<1> words and its ones
    uint64_t *lastw = dev.take<uint64_t>(nw);
    pack_bits_kernel<<<dim3(dbg_grid(nw)), dim3(256), 0, s>>>(ch.last, n, lastw);
    HIP_CHECK(hipGetLastError());
    const uint64_t nb_5 = (nw >> 5) + 1;
    uint64_t *rank_5 = dev.take<uint64_t>(2 * nb_5);
    {
        uint32_t *cnt = dev.take<uint32_t>(nb_5);
        uint64_t *sc = dev.take<uint64_t>(nb_5 + 1);
        rank_blocks_kernel<32><<<dim3(dbg_grid(nb_5)), dim3(kThreads), 0, s>>>(lastw, nw, nb_5, cnt, rank_5);
        HIP_CHECK(hipGetLastError());
        exclusive_scan(cnt, nb_5, sc, scan_tmp(nb_5), s);
        rank_first_kernel<<<dim3(dbg_grid(nb_5)), dim3(kThreads), 0, s>>>(sc, nb_5, rank_5);
        HIP_CHECK(hipGetLastError());
        GatherIdx g{};
        g.idx[0] = nb_5;
        gather_kernel<<<dim3(1), dim3(64), 0, s>>>(sc, g, 1, d_small + S_ONES);
        HIP_CHECK(hipGetLastError());
    }

    // 5. the navigation directory
    Nav nav{};
    if (navigate) nav = build_nav(dev, s, ch.W, lastw, n, k, ch.F, d_small + S_NAV, h_small + S_NAV);

    // 6. the suffix-range index, one level per char
    uint64_t n_ranges = 0;
    uint64_t *ranges = nullptr;
    if (L) {
        n_ranges = 1ull << (2 * L);
        uint64_t *a = dev.take<uint64_t>(2 * n_ranges), *b = dev.take<uint64_t>(2 * n_ranges);
        suffix_root_kernel<<<dim3(1), dim3(64), 0, s>>>(n, a);
        HIP_CHECK(hipGetLastError());
        uint64_t num = 1;
        for (uint64_t len = 1; len <= L; ++len, num *= 4) {
            suffix_level_kernel<<<dim3(dbg_grid(4 * num)), dim3(kThreads), 0, s>>>(nav, a, num, b);
            HIP_CHECK(hipGetLastError());
            std::swap(a, b);
        }
        ranges = a;
    }

    // 7. the valid-edge mask
    uint64_t *maskw = nullptr;
    if (mask_dummy) {
        const uint8_t *flagged = flagged_in;
        uint8_t *walked = flagged_in ? nullptr : dev.take<uint8_t>(n);
        if (walked) {
            HIP_CHECK(hipMemsetAsync(walked, 0, n, s));
            flagged = walked;
        }
        if (walked && n > 1)
            walk_source_dummies(dev, s, nav, d_small + S_NAV + 5, h_small + S_COUNT, walked, "write_dbg_device");
        maskw = dev.take<uint64_t>(nw);
        mask_pack_kernel<<<dim3(dbg_grid(nw)), dim3(kThreads), 0, s>>>(ch.W, flagged, n, nw, maskw,
                                                                    (unsigned long long *)(d_small + S_NVALID));
        HIP_CHECK(hipGetLastError());
    }

    // 8. the weights' int_vector words
    const uint64_t nww = weighted ? ceil_div(n * bits_per_count, 64) : 0;
    uint64_t *wwords = nullptr;
    if (weighted) {
        wwords = dev.take<uint64_t>(nww);
        weights_pack_kernel<<<dim3(dbg_grid(nww)), dim3(kThreads), 0, s>>>(ch.weights, n, bits_per_count, nww, wwords);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(ev[1], s));

    // payloads -> pinned host blocks
    HIP_CHECK(hipEventSynchronize(ev[1]));
    const auto t_d2h = std::chrono::steady_clock::now();
    uint64_t d2h_bytes = 0;
    auto fetch = [&](const uint64_t *d, uint64_t words) {
        uint64_t *h = pin.take<uint64_t>(words);
        if (words) HIP_CHECK(hipMemcpyAsync(h, d, words * 8, hipMemcpyDeviceToHost, s));
        d2h_bytes += words * 8;
        return h;
    };
    uint64_t *h_bv = fetch(bv, bvw);
    uint64_t *h_rank_v = fetch(rank_v, 2 * nb_v);
    uint64_t *h_last = fetch(lastw, nw);
    uint64_t *h_rank_5 = fetch(rank_5, 2 * nb_5);
    uint64_t *h_ranges = L ? fetch(ranges, 2 * n_ranges) : nullptr;
    uint64_t *h_mask = mask_dummy ? fetch(maskw, nw) : nullptr;
    uint64_t *h_weights = weighted ? fetch(wwords, nww) : nullptr;
    HIP_CHECK(hipMemcpyAsync(h_small + S_NVALID, d_small + S_NVALID, 2 * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const double d2h_ms = ms_since(t_d2h);
    float device_ms = 0;
    HIP_CHECK(hipEventElapsedTime(&device_ms, ev[0], ev[1]));

    // host: the inner nodes' ranks from the rank words, the forward fill, the files
    const auto t_host = std::chrono::steady_clock::now();
    wt.bv = h_bv;
    wt.rank = h_rank_v;
    wt.rank_words = 2 * nb_v;
    for (auto &v : wt.tree.nodes)
        if (v.child[0] != 0xFFFF) v.bv_pos_rank = sdslio::rank_v_query(h_bv, h_rank_v, v.bv_pos);
    P.last = h_last;
    P.last_ones = h_small[S_ONES];
    P.last_rank = h_rank_5;
    P.last_rank_words = 2 * nb_5;
    if (L) {
        dbgio::fill_empty_ranges(h_ranges, n_ranges);
        P.ranges = h_ranges;
        P.n_ranges = n_ranges;
    }
    if (mask_dummy) {
        P.valid = h_mask;
        P.n_valid = h_small[S_NVALID];
    }
    if (weighted) {
        P.weights = h_weights;
        P.weight_width = bits_per_count;
    }
    double stage_ms[5] = {0, 0, 0, 0, 0};
    const uint64_t n_valid = dbgio::write_dbg_payload(base, P, ch.F, k, mode, stage_ms);
    if (ctx.knobs.trace)
        fprintf(stderr, "[mtg trace] write_dbg_device host: wt_huff %.1f ms, last %.1f ms, index+framing %.1f ms, "
                        "edgemask %.1f ms, weights %.1f ms\n",
                stage_ms[0], stage_ms[1], stage_ms[2], stage_ms[3], stage_ms[4]);
    if (T) {
        T->device_ms = device_ms + pre_device_ms;
        T->d2h_ms = d2h_ms;
        T->host_ms = ms_since(t_host);
        T->d2h_bytes = d2h_bytes;
    }
    return n_valid;
}

uint64_t write_dbg_device_impl(Ctx &ctx, const mtg_boss_device_chunk &ch, unsigned bits_per_count,
                               const std::string &base, uint64_t mode, int mask_dummy, int64_t suffix_length,
                               mtg_dbg_write_timings *T) {
    return write_dbg_device_stages(ctx, ch, bits_per_count, base, mode, mask_dummy, suffix_length, T, nullptr, 0);
}

unsigned tile_grid(uint64_t n) {
    const uint64_t g = std::max<uint64_t>(dbgdev::state_tiles(n), 1);
    if (g > 0x7FFFFFFFull) throw std::runtime_error("write_dbg_device: too many rows for one launch");
    return (unsigned)g;
}

// BOSS::erase_edges on the stream: the rows of (W, last, aux) with erase[i] == 0 go to the *_out arrays
// (n bytes each; aux may be null), d_out[0] = the kept rows, d_out[1..5] = their F.  No synchronisation.
void erase_rows_device(DevScratch &dev, hipStream_t s, const uint8_t *W, const uint8_t *last, const uint8_t *aux,
                       const uint8_t *erase, uint64_t n, const uint64_t *F, uint8_t *W_out, uint8_t *last_out,
                       uint8_t *aux_out, uint64_t *d_out) {
    using namespace dbgdev;
    const unsigned grid = tile_grid(n);
    uint32_t *tstate = dev.take<uint32_t>(grid);
    uint64_t *tcount = dev.take<uint64_t>(grid);
    FVec f{};
    for (int c = 0; c < 5; ++c) f.F[c] = std::min<uint64_t>(F[c], n - 1);
    state_tile_kernel<kErase><<<dim3(grid), dim3(kThreads), 0, s>>>(W, erase, n, tstate, tcount);
    HIP_CHECK(hipGetLastError());
    state_carry_kernel<<<dim3(1), dim3(kThreads), 0, s>>>(tstate, tcount, grid, d_out);
    HIP_CHECK(hipGetLastError());
    for (int pass = 0; pass < 2; ++pass) {
        erase_apply_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(W, last, aux, erase, n, tstate, tcount, f, pass, W_out,
                                                                last_out, aux_out, d_out + 1);
        HIP_CHECK(hipGetLastError());
    }
}

// mtg_boss_erase_edges_device
void erase_edges_device_impl(Ctx &ctx, const mtg_boss_device_chunk &in, const uint8_t *d_erase,
                             mtg_boss_device_chunk *out) {
    hipStream_t s = ctx.stream;
    PinnedBlocks pin;
    DevScratch dev;
    uint64_t *h = pin.take<uint64_t>(8);
    HIP_CHECK(hipMemcpyAsync(h, d_erase, 1, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (*(const uint8_t *)h) throw DbgArgumentError("erase_edges_device: row 0 cannot be erased");
    uint64_t *d_out = dev.take<uint64_t>(8);
    erase_rows_device(dev, s, in.W, in.last, nullptr, d_erase, in.n, in.F, out->W, out->last, nullptr, d_out);
    HIP_CHECK(hipMemcpyAsync(h, d_out, 6 * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    out->k = in.k;
    out->n = h[0];
    for (int c = 0; c < 5; ++c) out->F[c] = h[1 + c];
}

// mtg_boss_write_dbg_device_pruned: dbgio::write_dbg's mask_dummy == 2 branch on a device chunk
uint64_t write_dbg_device_pruned_impl(Ctx &ctx, const mtg_boss_device_chunk &ch, const std::string &base,
                                      uint64_t mode, int64_t suffix_length, uint64_t *n_erased,
                                      mtg_dbg_write_timings *T) {
    using namespace dbgdev;
    hipStream_t s = ctx.stream;
    const uint64_t n = ch.n, nw = ceil_div(n, 64), k = ch.k;
    PinnedBlocks pin;
    DevScratch dev;
    hipEvent_t ev[2];
    for (auto &e : ev) HIP_CHECK(hipEventCreate(&e));
    struct EvGuard {
        hipEvent_t *ev;
        ~EvGuard() {
            for (int i = 0; i < 2; ++i) (void)hipEventDestroy(ev[i]);
        }
    } ev_guard{ev};
    HIP_CHECK(hipEventRecord(ev[0], s));
    uint64_t *d_small = dev.take<uint64_t>(16);
    uint64_t *h_small = pin.take<uint64_t>(16);

    // the navigation directory of the input
    uint64_t *lastw = dev.take<uint64_t>(nw);
    pack_bits_kernel<<<dim3(dbg_grid(nw)), dim3(256), 0, s>>>(ch.last, n, lastw);
    HIP_CHECK(hipGetLastError());
    const Nav nav = build_nav(dev, s, ch.W, lastw, n, k, ch.F, d_small, h_small);

    // the single-incoming flags
    const unsigned grid = tile_grid(n);
    uint8_t *single = dev.take<uint8_t>(n);
    {
        uint32_t *tstate = dev.take<uint32_t>(grid);
        state_tile_kernel<kSingle><<<dim3(grid), dim3(kThreads), 0, s>>>(ch.W, nullptr, n, tstate, nullptr);
        HIP_CHECK(hipGetLastError());
        state_carry_kernel<<<dim3(1), dim3(kThreads), 0, s>>>(tstate, nullptr, grid, nullptr);
        HIP_CHECK(hipGetLastError());
        single_apply_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(ch.W, n, tstate, single);
        HIP_CHECK(hipGetLastError());
    }

    // the walk down, every level kept in one pool of n entries
    uint8_t *source = dev.take<uint8_t>(n), *erase = dev.take<uint8_t>(n);
    HIP_CHECK(hipMemsetAsync(source, 0, n, s));
    HIP_CHECK(hipMemsetAsync(erase, 0, n, s));
    if (n > 1) HIP_CHECK(hipMemsetAsync(source + 1, 1, 1, s));
    prune_roots_kernel<<<dim3(1), dim3(64), 0, s>>>(nav, d_small + 8);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_small + 8, d_small + 8, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t m = h_small[8];
    if (m > n) throw DbgArgumentError("write_dbg_device_pruned: the arrays are no BOSS table");
    if (m) {
        uint64_t *edge = dev.take<uint64_t>(n), *parent = dev.take<uint64_t>(n);
        uint8_t *needed = dev.take<uint8_t>(n);
        DevScratch::Buf *fb = dev.make(), *cb = dev.make(), *sb = dev.make(), *tb = dev.make();
        prune_root_level_kernel<<<dim3(dbg_grid(m)), dim3(kThreads), 0, s>>>(m, edge, parent);
        HIP_CHECK(hipGetLastError());
        std::vector<std::pair<uint64_t, uint64_t>> levels;  // (offset in the pool, entries)
        uint64_t off = 0;
        for (uint64_t depth = 1;; ++depth) {
            uint64_t *first = DevScratch::ensure<uint64_t>(fb, m);
            uint32_t *cnt = DevScratch::ensure<uint32_t>(cb, m);
            prune_visit_kernel<<<dim3(dbg_grid(m)), dim3(kThreads), 0, s>>>(nav, single, edge + off, m, depth == k ? 1 : 0,
                                                                          source, needed + off, first, cnt);
            HIP_CHECK(hipGetLastError());
            levels.push_back({off, m});
            if (depth >= k) break;
            uint64_t *sc = DevScratch::ensure<uint64_t>(sb, m + 1);
            exclusive_scan(cnt, m, sc, DevScratch::ensure<uint64_t>(tb, ceil_div(m, kScanTile) + 1), s);
            HIP_CHECK(hipMemcpyAsync(h_small + 8, sc + m, 8, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            const uint64_t next_m = h_small[8];
            if (next_m > n || off + m + next_m > n)
                throw DbgArgumentError("write_dbg_device_pruned: the arrays are no BOSS table (the source-dummy tree "
                                       "outgrows the rows)");
            if (!next_m) break;
            prune_expand_kernel<<<dim3(dbg_grid(m)), dim3(kThreads), 0, s>>>(first, cnt, sc, m, edge + off + m,
                                                                           parent + off + m, next_m);
            HIP_CHECK(hipGetLastError());
            off += m;
            m = next_m;
        }
        // needed, from the deepest level up; then the redundant rows
        for (size_t d = levels.size(); d-- > 1;) {
            const uint64_t o = levels[d].first, c = levels[d].second;
            prune_up_kernel<<<dim3(dbg_grid(c)), dim3(kThreads), 0, s>>>(needed + o, parent + o, c,
                                                                       needed + levels[d - 1].first, levels[d - 1].second);
            HIP_CHECK(hipGetLastError());
        }
        const uint64_t total = levels.back().first + levels.back().second;
        prune_mark_kernel<<<dim3(dbg_grid(total)), dim3(kThreads), 0, s>>>(edge, needed, total, n, erase);
        HIP_CHECK(hipGetLastError());
    }

    // erase_edges, the source flags carried along
    uint8_t *W2 = dev.take<uint8_t>(n), *last2 = dev.take<uint8_t>(n), *source2 = dev.take<uint8_t>(n);
    erase_rows_device(dev, s, ch.W, ch.last, source, erase, n, ch.F, W2, last2, source2, d_small + 8);
    HIP_CHECK(hipMemcpyAsync(h_small + 8, d_small + 8, 6 * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(ev[1], s));
    HIP_CHECK(hipStreamSynchronize(s));
    float prune_ms = 0;
    HIP_CHECK(hipEventElapsedTime(&prune_ms, ev[0], ev[1]));
    mtg_boss_device_chunk pruned{};
    pruned.k = k;
    pruned.n = h_small[8];
    pruned.W = W2;
    pruned.last = last2;
    for (int c = 0; c < 5; ++c) pruned.F[c] = h_small[9 + c];
    if (pruned.n < 1 || pruned.n > n) throw std::runtime_error("write_dbg_device_pruned: bad row count after erase");
    if (n_erased) *n_erased = n - pruned.n;
    if (ctx.knobs.trace)
        fprintf(stderr, "[mtg trace] write_dbg_device_pruned: %llu of %llu rows erased, prune %.2f ms\n",
                (unsigned long long)(n - pruned.n), (unsigned long long)n, prune_ms);
    // the pruned graph and its mask; no weights file, as build_boss_from_chunks takes none
    return write_dbg_device_stages(ctx, pruned, 0, base, mode, 1, suffix_length, T, source2, prune_ms);
}

// mtg_boss_chunk_extend_device: BOSS::Chunk::extend (boss_chunk.cpp:230-270) on caller-owned device arrays
void chunk_extend_device_impl(Ctx &ctx, mtg_boss_device_chunk *dst, uint64_t capacity, const mtg_boss_device_chunk &src) {
    hipStream_t s = ctx.stream;
    const bool empty = dst->n == 0;  // a buffer without rows takes src whole, row 0 included
    if (!empty && src.n == 1) return;
    const uint64_t from = empty ? 0 : 1, rows = src.n - from;
    if (dst->n + rows > capacity) throw DbgArgumentError("chunk_extend_device: the destination's capacity is too small");
    HIP_CHECK(hipMemcpyAsync(dst->W + dst->n, src.W + from, rows, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(dst->last + dst->n, src.last + from, rows, hipMemcpyDeviceToDevice, s));
    if (dst->weights)
        HIP_CHECK(hipMemcpyAsync(dst->weights + dst->n, src.weights + from, rows * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dst->n += rows;
    for (int c = 0; c < 5; ++c) dst->F[c] = (empty ? 0 : dst->F[c]) + src.F[c];
    dst->n_real = (empty ? 0 : dst->n_real) + src.n_real;
    dst->n_dummy = (empty ? 0 : dst->n_dummy) + src.n_dummy;
}

}  // namespace

}  // namespace mtg
