// unitigs_device.hpp -- the host driver of unitigs.hpp and the writer of its output as the pair
// ExtendedFastaWriter writes (seq_io/sequence_io.cpp:91-183): <base>.fasta.gz and <base>.kmer_counts.gz.
// Included by boss_pipeline.hip only, after dbg_device_write.hpp (its scratch, navigation directory and
// source-dummy walk) and ahead of the C ABI.
#pragma once

#include <zlib.h>

#include "dbg_device_write.hpp"
#include "unitigs.hpp"

namespace mtg {
namespace {

struct UnitigRun {
    uint64_t rank_rounds = 0;   // doubling rounds of the ranking, both passes
    uint64_t cycle_rounds = 0;  // rounds of the closed chains' minimum search
    double device_ms = 0;
};

void free_unitigs(mtg_device_unitigs *u) {
    if (u->seq) (void)hipFree(u->seq);
    if (u->record_starts) (void)hipFree(u->record_starts);
    if (u->kmer_counts) (void)hipFree(u->kmer_counts);
    u->seq = nullptr;
    u->record_starts = nullptr;
    u->kmer_counts = nullptr;
}

// mtg_boss_unitigs_device: the chunk is only read; out's three arrays are hipMalloc'ed here
void unitigs_device_impl(Ctx &ctx, const mtg_boss_device_chunk &ch, const mtg_unitig_params &prm,
                         mtg_device_unitigs *out, UnitigRun *run) {
    using namespace dbgdev;
    using namespace unitig;
    hipStream_t s = ctx.stream;
    const uint64_t n = ch.n, nw = ceil_div(n, 64), k = ch.k, K = k + 1;
    const bool weighted = ch.weights != nullptr;
    const bool filter_weak = prm.min_median_abundance > 1;
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
    enum { S_NAV = 0, S_COUNT = 6, S_FLAG = 7, S_DROPPED = 8, S_TOTALS = 10, S_WORDS = 12 };
    uint64_t *d_small = dev.take<uint64_t>(S_WORDS);
    uint64_t *h_small = pin.take<uint64_t>(S_WORDS);
    HIP_CHECK(hipMemsetAsync(d_small, 0, S_WORDS * 8, s));
    const unsigned grid = dbg_grid(n);

    // 1. the real-edge flags: the navigation directory, the source-dummy walk of the graph writer
    uint64_t *lastw = dev.take<uint64_t>(nw);
    pack_bits_kernel<<<dim3(dbg_grid(nw)), dim3(256), 0, s>>>(ch.last, n, lastw);
    HIP_CHECK(hipGetLastError());
    const Nav nav = build_nav(dev, s, ch.W, lastw, n, k, ch.F, d_small + S_NAV, h_small + S_NAV);
    uint8_t *source = dev.take<uint8_t>(n), *real = dev.take<uint8_t>(n);
    HIP_CHECK(hipMemsetAsync(source, 0, n, s));
    if (n > 1) walk_source_dummies(dev, s, nav, d_small + S_NAV + 5, h_small + S_COUNT, source, "unitigs_device");
    unitig_real_kernel<<<dim3(dbg_grid(ceil_div(n, 16))), dim3(kThreads), 0, s>>>(ch.W, source, n, real);
    HIP_CHECK(hipGetLastError());

    // 2. degrees and links
    uint32_t *tgt = dev.take<uint32_t>(n), *indeg = dev.take<uint32_t>(n);
    uint32_t *succ = dev.take<uint32_t>(n), *pred = dev.take<uint32_t>(n);
    uint8_t *outdeg_k = dev.take<uint8_t>(n), *indeg_k = dev.take<uint8_t>(n);
    HIP_CHECK(hipMemsetAsync(indeg, 0, n * 4, s));
    HIP_CHECK(hipMemsetAsync(succ, 0xFF, n * 4, s));
    HIP_CHECK(hipMemsetAsync(pred, 0xFF, n * 4, s));
    HIP_CHECK(hipMemsetAsync(outdeg_k, 0, n, s));
    HIP_CHECK(hipMemsetAsync(indeg_k, 0, n, s));
    unitig_target_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(nav, real, tgt, indeg);
    HIP_CHECK(hipGetLastError());
    unitig_link_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(real, ch.last, n, tgt, indeg, succ, pred, outdeg_k, indeg_k);
    HIP_CHECK(hipGetLastError());

    // 3. ranking: doubling rounds until nothing moves, the host reads one word per round
    uint32_t *d_flag = (uint32_t *)(d_small + S_FLAG);
    uint64_t max_rounds = 1;
    while ((1ull << (max_rounds - 1)) < n) ++max_rounds;  // ceil(log2 n) + 1
    auto read_flag = [&]() {
        HIP_CHECK(hipMemcpyAsync(h_small + S_FLAG, d_flag, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        return *(const uint32_t *)(h_small + S_FLAG) != 0;
    };
    uint64_t *sa = dev.take<uint64_t>(n), *sb = dev.take<uint64_t>(n);
    // true when the rounds stopped by themselves; the state is in sa afterwards
    auto rank = [&]() {
        for (uint64_t r = 0; r < max_rounds; ++r) {
            HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, s));
            unitig_rank_round_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(sa, n, sb, d_flag);
            HIP_CHECK(hipGetLastError());
            std::swap(sa, sb);
            ++run->rank_rounds;
            if (!read_flag()) return true;
        }
        return false;
    };
    unitig_rank_init_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(pred, n, nullptr, sa);
    HIP_CHECK(hipGetLastError());
    if (!rank()) {
        // closed chains: their smallest rows become first k-mers, then those rows are ranked again
        uint8_t *cyc = dev.take<uint8_t>(n);
        uint64_t *ma = dev.take<uint64_t>(n), *mb = dev.take<uint64_t>(n);
        HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, s));
        unitig_cycle_init_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(sa, pred, n, cyc, ma, d_flag);
        HIP_CHECK(hipGetLastError());
        if (read_flag()) {
            for (uint64_t r = 0; r < max_rounds; ++r) {
                HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, s));
                unitig_cycle_round_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(ma, n, mb, d_flag);
                HIP_CHECK(hipGetLastError());
                std::swap(ma, mb);
                ++run->cycle_rounds;
                if (!read_flag()) break;
            }
            unitig_cycle_cut_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(cyc, ma, n, succ, pred);
            HIP_CHECK(hipGetLastError());
            unitig_rank_init_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(pred, n, cyc, sa);
            HIP_CHECK(hipGetLastError());
            if (!rank()) throw DbgArgumentError("unitigs_device: the arrays are no BOSS table (the links do not form chains)");
        }
    }

    // 4. per-unitig statistics, the filters, the offsets
    uint32_t *tail = dev.take<uint32_t>(n), *len = dev.take<uint32_t>(n), *weak = dev.take<uint32_t>(n);
    uint32_t *klen = tgt, *kflag = indeg;  // both free since the links
    HIP_CHECK(hipMemsetAsync(tail, 0xFF, n * 4, s));
    HIP_CHECK(hipMemsetAsync(len, 0, n * 4, s));
    HIP_CHECK(hipMemsetAsync(weak, 0, n * 4, s));
    unitig_stats_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(real, sa, succ, n, ch.weights, prm.min_median_abundance, tail,
                                                           len, weak);
    HIP_CHECK(hipGetLastError());
    unitig_filter_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(real, sa, n, tail, len, weak, outdeg_k, indeg_k,
                                                            prm.min_tip_size, filter_weak ? 1 : 0, klen, kflag,
                                                            (unsigned long long *)(d_small + S_DROPPED));
    HIP_CHECK(hipGetLastError());
    uint64_t *cnt_off = dev.take<uint64_t>(n + 1), *rec_idx = dev.take<uint64_t>(n + 1);
    uint64_t *scan_tmp = dev.take<uint64_t>(ceil_div(n, kScanTile) + 1);
    exclusive_scan(klen, n, cnt_off, scan_tmp, s);
    exclusive_scan(kflag, n, rec_idx, scan_tmp, s);
    HIP_CHECK(hipMemcpyAsync(d_small + S_TOTALS, cnt_off + n, 8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_small + S_TOTALS + 1, rec_idx + n, 8, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(h_small + S_DROPPED, d_small + S_DROPPED, 4 * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    out->n_dropped_records = h_small[S_DROPPED];
    out->n_dropped_kmers = h_small[S_DROPPED + 1];
    out->n_kmers = h_small[S_TOTALS];
    out->n_records = h_small[S_TOTALS + 1];
    if (out->n_kmers > n || out->n_records > out->n_kmers)
        throw std::runtime_error("unitigs_device: bad totals after the scans");
    out->seq_len = out->n_kmers + out->n_records * K;

    // 5. emit
    HIP_CHECK(hipMalloc(&out->seq, std::max<uint64_t>(out->seq_len, 1)));
    HIP_CHECK(hipMalloc(&out->record_starts, (out->n_records + 1) * 8));
    if (weighted) HIP_CHECK(hipMalloc(&out->kmer_counts, std::max<uint64_t>(out->n_kmers, 1) * 4));
    EmitOut eo{};
    eo.seq = out->seq;
    eo.seq_len = out->seq_len;
    eo.record_starts = out->record_starts;
    eo.n_records = out->n_records;
    eo.counts = out->kmer_counts;
    eo.n_kmers = out->n_kmers;
    eo.K = K;
    unitig_emit_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(ch.W, real, sa, n, kflag, cnt_off, rec_idx, ch.weights, eo);
    HIP_CHECK(hipGetLastError());
    unitig_emit_heads_kernel<<<dim3(grid), dim3(kThreads), 0, s>>>(nav, kflag, klen, cnt_off, rec_idx, eo);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev[1], s));
    HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    run->device_ms = ms;
    if (ctx.knobs.trace)
        fprintf(stderr, "[mtg trace] unitigs_device: %llu rows -> %llu records, %llu k-mers (%llu + %llu dropped), "
                        "%llu ranking rounds, %llu closed-chain rounds, %.2f ms\n",
                (unsigned long long)n, (unsigned long long)out->n_records, (unsigned long long)out->n_kmers,
                (unsigned long long)out->n_dropped_records, (unsigned long long)out->n_dropped_kmers,
                (unsigned long long)run->rank_rounds, (unsigned long long)run->cycle_rounds, ms);
}

// mtg_boss_write_unitigs_device: both files are opened before anything is written; a failure removes them
void write_unitigs_files(Ctx &ctx, const mtg_device_unitigs &u, uint64_t K, const std::string &base, bool weighted) {
    hipStream_t s = ctx.stream;
    PinnedBlocks pin;
    uint8_t *seq = pin.take<uint8_t>(u.seq_len);
    uint64_t *rs = pin.take<uint64_t>(u.n_records + 1);
    uint32_t *cnt = weighted ? pin.take<uint32_t>(u.n_kmers) : nullptr;
    if (u.seq_len) HIP_CHECK(hipMemcpyAsync(seq, u.seq, u.seq_len, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(rs, u.record_starts, (u.n_records + 1) * 8, hipMemcpyDeviceToHost, s));
    if (weighted && u.n_kmers) HIP_CHECK(hipMemcpyAsync(cnt, u.kmer_counts, u.n_kmers * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));

    const std::string fa_name = base + ".fasta.gz", kc_name = base + ".kmer_counts.gz";
    gzFile fa = gzopen(fa_name.c_str(), "w");
    if (fa == Z_NULL) throw std::runtime_error("ERROR: Can't write to " + fa_name);
    gzFile kc = Z_NULL;
    if (weighted) {
        kc = gzopen(kc_name.c_str(), "w");
        if (kc == Z_NULL) {
            gzclose(fa);
            std::remove(fa_name.c_str());
            throw std::runtime_error("ERROR: Can't write to " + kc_name);
        }
    }
    bool ok = true;
    auto put = [&](gzFile f, const void *p, uint64_t bytes) {
        const uint8_t *b = (const uint8_t *)p;
        while (ok && bytes) {
            const unsigned piece = (unsigned)std::min<uint64_t>(bytes, 1u << 30);
            ok = gzwrite(f, b, piece) == (int)piece;
            b += piece;
            bytes -= piece;
        }
    };
    std::string buf;
    buf.reserve((1u << 20) + 64);
    for (uint64_t r = 0; r < u.n_records && ok; ++r) {
        if (rs[r + 1] <= rs[r] || rs[r + 1] > u.seq_len) {
            ok = false;
            break;
        }
        buf += '>';
        buf += std::to_string(r + 1);
        buf += '\n';
        buf.append((const char *)seq + rs[r], rs[r + 1] - 1 - rs[r]);  // without the separator
        buf += '\n';
        if (buf.size() >= (1u << 20)) {
            put(fa, buf.data(), buf.size());
            buf.clear();
        }
    }
    put(fa, buf.data(), buf.size());
    if (weighted) {
        const uint32_t kmer_length = (uint32_t)K;
        put(kc, &kmer_length, 4);
        put(kc, cnt, u.n_kmers * 4);
    }
    ok = (gzclose(fa) == Z_OK) && ok;
    if (weighted) ok = (gzclose(kc) == Z_OK) && ok;
    if (!ok) {
        std::remove(fa_name.c_str());
        if (weighted) std::remove(kc_name.c_str());
        throw std::runtime_error("ERROR: Can't dump the unitigs to " + fa_name);
    }
}

}  // namespace
}  // namespace mtg
