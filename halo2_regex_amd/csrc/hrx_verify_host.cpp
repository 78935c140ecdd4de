// hrx_verify_host.cpp — the host form of VERIFY (include/hrx.h hrx_verify_rows_host): the rules of hrx_verify.hpp over rows in host memory, string-major
// (tight or pitched) or position-major as copied from the device, over threads by ranges of strings.  No HIP, no allocation; the host twin of
// hrx_kernel_verify.hip and the definition of the verdict word's row field.  tests/host_cpp/test_verify_host.cpp includes this file as it is.
// verify_rows_chunked_host is the host form of the chunked rule (hrx_verify_rows_chunked_host): threads over (string, chunk) pairs, then the fold per string.
#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

#include "hrx_verify.hpp"

namespace hrx {

namespace {

// string b of a batch in host memory (the address rules of include/hrx.h, as hrx_witness_columns_host reads them)
struct HostRows {
    const VerifyArgs &a;
    size_t b, k, bl, nb, q4, q8;
    bool pm, in_pm;
    HostRows(const VerifyArgs &args, size_t string) : a(args), b(string) {
        k = b / kVfyPmBlock; bl = b % kVfyPmBlock; nb = std::min<size_t>(kVfyPmBlock, a.B - k * kVfyPmBlock);
        q4 = ((size_t)a.M + 3) / 4; q8 = ((size_t)a.M + 7) / 8;
        pm = (a.layout & 1u) != 0; in_pm = (a.layout & 2u) != 0;
    }
    uint32_t chr(size_t i) const { return in_pm ? a.chars[k * kVfyPmBlock * a.stride + ((i / 16) * nb + bl) * 16 + i % 16] : a.chars[b * a.stride + i]; }
    uint32_t rec(size_t r, size_t d) const {
        return pm ? a.records[k * kVfyPmBlock * q4 * a.D * 4 + ((r / 4 * a.D + d) * nb + bl) * 4 + r % 4] : a.records[(b * a.rec_pitch + r) * a.D + d];
    }
    uint32_t msk(size_t r) const { return pm ? a.masked[k * kVfyPmBlock * q8 * 8 + (r / 8 * nb + bl) * 8 + r % 8] : a.masked[b * a.msk_pitch + r]; }
};

void verify_range(const VerifyArgs &a, size_t b0, size_t b1) {
    for (size_t b = b0; b < b1; ++b) a.verdict[b] = verify_string(a.image, a.D, a.lens[b], a.M, HostRows(a, b));
}

}  // namespace

// arguments checked by the caller (a.image: build_verify_image of the config, in host memory).  threads: 0 = as many as the machine has, at most 16;
// never more than one per 64 strings
void verify_rows_host(const VerifyArgs &a, unsigned threads) {
    if (a.B == 0 || a.M == 0) return;
    if (threads == 0) threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    threads = (unsigned)std::min<size_t>(threads, ((size_t)a.B + 63) / 64);
    if (threads <= 1) return verify_range(a, 0, a.B);
    const size_t per = ((size_t)a.B + threads - 1) / threads;
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < threads; ++t) {
        const size_t b0 = std::min<size_t>(a.B, t * per), b1 = std::min<size_t>(a.B, b0 + per);
        if (b0 < b1) pool.emplace_back(verify_range, std::cref(a), b0, b1);
    }
    verify_range(a, 0, std::min<size_t>(a.B, per));
    for (std::thread &t : pool) t.join();
}

namespace {

// fn(i0, i1) over [0, count) on `threads` threads
template <class Fn>
void over_threads(size_t count, unsigned threads, const Fn &fn) {
    threads = (unsigned)std::min<size_t>(threads, count);
    if (threads <= 1) return fn((size_t)0, count);
    const size_t per = (count + threads - 1) / threads;
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < threads; ++t) {
        const size_t i0 = std::min(count, t * per), i1 = std::min(count, i0 + per);
        if (i0 < i1) pool.emplace_back(fn, i0, i1);
    }
    fn((size_t)0, std::min(count, per));
    for (std::thread &t : pool) t.join();
}

}  // namespace

// The chunked rule on the host (hrx_verify_rows_chunked_host): verify_chunk_string over (string, chunk) pairs — so a few long strings still use every
// thread — into summaries laid out as the kernel's ([field][chunk][string]), then verify_fold_chunk per string.  `summaries`: [kVfyChunkFields][K][B] u32.
// chunk_rows: a multiple of kVfyChunkAlign.
void verify_rows_chunked_host(const VerifyArgs &a, uint32_t chunk_rows, uint32_t *summaries, unsigned threads) {
    if (a.B == 0 || a.M == 0) return;
    if (threads == 0) threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    const size_t B = a.B, K = verify_chunk_count(a.M, chunk_rows);
    over_threads(B * K, threads, [&a, chunk_rows, summaries, B, K](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            const size_t b = i / K, k = i % K;
            if (a.lens[b] > a.M) continue;          // no rows: no chunk of the string reads one
            const uint32_t r0 = (uint32_t)k * chunk_rows, r1 = (uint32_t)std::min<size_t>(a.M, (size_t)r0 + chunk_rows);
            const VerifyChunk v = verify_chunk_string(a.image, a.D, a.lens[b], a.M, r0, r1, HostRows(a, b));
            const uint32_t w[kVfyChunkFields] = {v.flags, v.row, v.mask_row[0], v.mask_row[1], v.need1[0], v.need1[1], v.need0[0], v.need0[1]};
            for (size_t f = 0; f < kVfyChunkFields; ++f) summaries[(f * K + k) * B + b] = w[f];
        }
    });
    over_threads(B, std::min<unsigned>(threads, (unsigned)((B + 63) / 64)), [&a, summaries, B, K](size_t b0, size_t b1) {
        for (size_t b = b0; b < b1; ++b) {
            if (a.lens[b] > a.M) { a.verdict[b] = ~0ull; continue; }
            VerifyAcc acc;
            verify_begin(acc);
            for (size_t k = 0; k < K; ++k) {
                uint32_t w[kVfyChunkFields];
                for (size_t f = 0; f < kVfyChunkFields; ++f) w[f] = summaries[(f * K + k) * B + b];
                verify_fold_chunk(acc, VerifyChunk{w[0], w[1], {w[2], w[3]}, {w[4], w[5]}, {w[6], w[7]}});
            }
            a.verdict[b] = verify_finish(acc);
        }
    });
}

}  // namespace hrx
