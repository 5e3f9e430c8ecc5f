// chunk_host.hpp -- a chunk's way on and off the device: the staged reads unpacked to one byte per char, and
// the finished rows' trip to the host -- `last` packed to bits, W as 4-bit codes and narrow weights as 1 or 2
// bytes, copied in pieces into a pinned landing buffer that the host threads unpack while later pieces are
// still in flight.  Included by boss_pipeline.hip only, after ctx.hpp.
#pragma once

#include <immintrin.h>

#include "ctx.hpp"
#include "host_stage.hpp"

// The kernels keep the linkage they were written with, and so their symbols: the first two C++ names at
// global scope, the other two C names.

// staged reads (host_stage.hpp) -> one byte per char: ACGT, or 'N' for every char that breaks a
// k-mer window (separators, alignment gaps, N and the rest); one 32-char word per thread
__global__ void unpack_reads_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                    uint64_t nw, uint8_t *__restrict__ out) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const uint64_t c = codes[w];
    const uint32_t v = valid[w];
    uint32_t o[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * q + b;
            const uint32_t ch = (v >> j) & 1u ? (0x54474341u >> (8 * ((c >> (2 * j)) & 3u))) & 0xFFu : (uint32_t)'N';
            word |= ch << (8 * b);
        }
        o[q] = word;
    }
    uint4 *dst = (uint4 *)(out + 32 * w);
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// one packed `last` word per thread: bit j of word w = last[64 w + j] (sdsl bit_vector layout)
__global__ void pack_bits_kernel(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t *__restrict__ words) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i0 = w * 64;
    if (i0 >= n) return;
    uint64_t v = 0;
    if (i0 + 64 <= n && ((uintptr_t)(bytes + i0) & 7) == 0) {
        const uint64_t *p = reinterpret_cast<const uint64_t *>(bytes + i0);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint64_t x = p[q];  // 8 flag bytes (0/1) -> 8 bits
            v |= ((x * 0x0102040810204080ull) >> 56 & 0xFFull) << (8 * q);
        }
    } else {
        for (uint64_t j = 0; j < 64 && i0 + j < n; ++j) v |= (uint64_t)(bytes[i0 + j] & 1) << j;
    }
    words[w] = v;
}

extern "C" {

// W (values 0..9) crosses PCIe as 4-bit codes: packed on the device, copied in pieces, and
// unpacked by the host threads as the pieces land (half the bytes of the largest D2H)
__global__ void pack_w4_kernel(const uint8_t *__restrict__ w, uint64_t n, uint8_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // 16 output bytes each
    const uint64_t b0 = i * 32;
    if (b0 >= n) return;
    uint32_t o[4] = {0, 0, 0, 0};
    if (b0 + 32 <= n) {
        const uint4 a = *(const uint4 *)(w + b0), b = *(const uint4 *)(w + b0 + 16);
        const uint32_t in[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {  // 4 W bytes -> 2 packed bytes
            const uint32_t v = in[q];
            const uint32_t p = (v & 0xF) | ((v >> 4) & 0xF0) | (((v >> 16) & 0xF) << 8) | (((v >> 24) & 0xF) << 12);
            o[q / 2] |= p << (16 * (q & 1));
        }
    } else {
        for (uint64_t j = b0; j < n; ++j) {
            const uint32_t k = (uint32_t)(j - b0);
            o[k / 8] |= (uint32_t)(w[j] & 0xF) << (4 * (k % 8));
        }
    }
    const uint64_t nb = (n + 1) / 2, ob = b0 / 2;
    if (ob + 16 <= nb) {
        *(uint4 *)(out + ob) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        for (uint64_t j = ob; j < nb; ++j) out[j] = (uint8_t)(o[(j - ob) / 4] >> (8 * ((j - ob) % 4)));
    }
}

// u32 weights (already clamped to the count width) -> `bytes` (1 or 2) per weight, 16 weights a thread
__global__ void narrow_weights_kernel(const uint32_t *__restrict__ w, uint64_t n, unsigned bytes,
                                      uint8_t *__restrict__ out) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (i0 >= n) return;
    if (i0 + 16 <= n) {
        const uint4 *src = (const uint4 *)(w + i0);
        uint32_t v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 a = src[q];
            v[4 * q] = a.x, v[4 * q + 1] = a.y, v[4 * q + 2] = a.z, v[4 * q + 3] = a.w;
        }
        if (bytes == 1) {
            uint32_t o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                o[q] = (v[4 * q] & 0xFF) | (v[4 * q + 1] & 0xFF) << 8 | (v[4 * q + 2] & 0xFF) << 16 | v[4 * q + 3] << 24;
            *(uint4 *)(out + i0) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            uint32_t o[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = (v[2 * q] & 0xFFFF) | v[2 * q + 1] << 16;
            *(uint4 *)(out + 2 * i0) = make_uint4(o[0], o[1], o[2], o[3]);
            *(uint4 *)(out + 2 * i0 + 16) = make_uint4(o[4], o[5], o[6], o[7]);
        }
        return;
    }
    for (uint64_t i = i0; i < n; ++i) {
        out[bytes * i] = (uint8_t)w[i];
        if (bytes == 2) out[2 * i + 1] = (uint8_t)(w[i] >> 8);
    }
}

}  // extern "C"

namespace mtg {

__attribute__((target("avx2"))) static void unpack_w4_avx2(const uint8_t *in, uint64_t nbytes, uint8_t *out) {
    uint64_t i = 0;
    const __m256i m = _mm256_set1_epi8(0x0F);
    for (; i + 32 <= nbytes; i += 32) {
        const __m256i v = _mm256_loadu_si256((const __m256i *)(in + i));
        const __m256i lo = _mm256_and_si256(v, m), hi = _mm256_and_si256(_mm256_srli_epi16(v, 4), m);
        const __m256i a = _mm256_unpacklo_epi8(lo, hi), b = _mm256_unpackhi_epi8(lo, hi);
        _mm256_storeu_si256((__m256i *)(out + 2 * i), _mm256_permute2x128_si256(a, b, 0x20));
        _mm256_storeu_si256((__m256i *)(out + 2 * i + 32), _mm256_permute2x128_si256(a, b, 0x31));
    }
    for (; i < nbytes; ++i) {
        out[2 * i] = in[i] & 0xF;
        out[2 * i + 1] = in[i] >> 4;
    }
}

static void unpack_w4(const uint8_t *in, uint64_t nbytes, uint8_t *out) {
    if (__builtin_cpu_supports("avx2")) return unpack_w4_avx2(in, nbytes, out);
    for (uint64_t i = 0; i < nbytes; ++i) {
        out[2 * i] = in[i] & 0xF;
        out[2 * i + 1] = in[i] >> 4;
    }
}

// a pinned host buffer the packed bytes land in: kept for the life of its constructor, regrown (a quarter
// above the request) when a copy needs more
struct PinnedLanding {
    uint8_t *p = nullptr;
    uint64_t cap = 0;
    PinnedLanding() = default;
    PinnedLanding(const PinnedLanding &) = delete;
    PinnedLanding &operator=(const PinnedLanding &) = delete;
    ~PinnedLanding() {
        if (p) (void)hipHostFree(p);
    }
    uint8_t *reserve(uint64_t bytes) {
        if (cap < bytes) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            cap = 0;
            HIP_CHECK(hipHostMalloc((void **)&p, bytes + bytes / 4, hipHostMallocDefault));
            cap = bytes + bytes / 4;
        }
        return p;
    }
};

// d[0..nb) on the device -> h (pinned) in pieces of `piece` bytes with one event each; up to `threads` host
// threads wait for the pieces (thread t takes t, t + T, ...) and hand each landed piece to done(b0, len)
template <class Done>
static void copy_pieces_to_host(const uint8_t *d, uint64_t nb, uint8_t *h, uint64_t piece, hipStream_t s, int device,
                                unsigned threads, const char *failure, Done done) {
    const uint64_t np = ceil_div(nb, piece);
    struct Events {
        std::vector<hipEvent_t> ev;
        ~Events() {
            for (auto e : ev) (void)hipEventDestroy(e);
        }
    } events;
    std::vector<hipEvent_t> &ev = events.ev;
    ev.reserve(np);
    for (uint64_t p = 0; p < np; ++p) {
        const uint64_t b0 = p * piece, len = std::min(piece, nb - b0);
        hipEvent_t e;
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ev.push_back(e);
        HIP_CHECK(hipMemcpyAsync(h + b0, d + b0, len, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipEventRecord(e, s));
    }
    const unsigned T = std::max(1u, (unsigned)std::min<uint64_t>(threads, np));
    std::atomic<bool> failed{false};
    parallel_ranges(T, T, 1, [&](uint64_t t0, uint64_t t1) {
        DeviceGuard g(device);
        for (uint64_t t = t0; t < t1; ++t)
            for (uint64_t p = t; p < np; p += T) {
                if (hipEventSynchronize(ev[p]) != hipSuccess) {
                    failed = true;
                    return;
                }
                const uint64_t b0 = p * piece;
                done(b0, std::min(piece, nb - b0));
            }
    });
    if (failed) throw std::runtime_error(failure);
}

// W[0..n) on the device -> host W (out, n bytes): 4-bit pieces of 16 MiB (Knobs::d2h_piece), unpacked as
// they land
static void copy_w_to_host(Ctx &c, int device, unsigned threads, PinnedLanding &land, const uint8_t *dW, uint64_t n,
                           uint8_t *out) {
    if (!n) return;
    hipStream_t s = c.stream;
    // small W: one plain copy (the pieces' sync and thread costs do not pay)
    if (n < (c.knobs.d2h_piece_set ? 0 : 128ull << 20)) {
        HIP_CHECK(hipMemcpyAsync(out, dW, n, hipMemcpyDeviceToHost, s));
        return;
    }
    const uint64_t nb = (n + 1) / 2;
    uint8_t *d4 = (uint8_t *)c.ws.get(Workspace::W4, nb + 16);
    pack_w4_kernel<<<dim3((unsigned)ceil_div(ceil_div(n, 32), 256)), dim3(256), 0, s>>>(dW, n, d4);
    HIP_CHECK(hipGetLastError());
    const uint8_t *h4 = land.reserve(nb + 16);
    copy_pieces_to_host(d4, nb, land.p, c.knobs.d2h_piece, s, device, threads, "W copy to the host failed",
                        [&](uint64_t b0, uint64_t len) {
                            // the last packed byte of an odd n holds one W value
                            const uint64_t full = (b0 + len == nb && (n & 1)) ? len - 1 : len;
                            unpack_w4(h4 + b0, full, out + 2 * b0);
                            if (full < len) out[2 * (b0 + full)] = h4[b0 + full] & 0xF;
                        });
}

// weights[0..n) (u32) on the device -> the host's u32 array: for count widths <= 16 bits they cross
// PCIe as 1 or 2 bytes a weight (configs[4]'s 8-bit weights: 1.5 GB -> 0.39 GB), in 16 MiB pieces
// that the host threads widen as they land
static void copy_weights_to_host(Ctx &c, int device, unsigned threads, PinnedLanding &land, const uint32_t *dwt,
                                 uint64_t n, unsigned bits, uint32_t *out) {
    if (!n) return;
    hipStream_t s = c.stream;
    const unsigned bytes = bits <= 8 ? 1 : bits <= 16 ? 2 : 4;
    if (bytes == 4 || n < (c.knobs.d2h_piece_set ? 0 : 16ull << 20)) {
        HIP_CHECK(hipMemcpyAsync(out, dwt, n * 4, hipMemcpyDeviceToHost, s));
        return;
    }
    const uint64_t nb = n * bytes;
    uint8_t *dn = (uint8_t *)c.ws.get(Workspace::WN, nb + 64);
    narrow_weights_kernel<<<dim3((unsigned)ceil_div(ceil_div(n, 16), 256)), dim3(256), 0, s>>>(dwt, n, bytes, dn);
    HIP_CHECK(hipGetLastError());
    const uint8_t *hn = land.reserve(nb + 64);
    // a piece is a multiple of 64 bytes: whole weights
    copy_pieces_to_host(dn, nb, land.p, c.knobs.d2h_piece, s, device, threads, "weights copy to the host failed",
                        [&](uint64_t b0, uint64_t len) {
                            const uint64_t w0 = b0 / bytes, wn = len / bytes;
                            if (bytes == 1)
                                for (uint64_t i = 0; i < wn; ++i) out[w0 + i] = hn[b0 + i];
                            else
                                for (uint64_t i = 0; i < wn; ++i)
                                    out[w0 + i] = (uint32_t)hn[b0 + 2 * i] | (uint32_t)hn[b0 + 2 * i + 1] << 8;
                        });
}

}  // namespace mtg
