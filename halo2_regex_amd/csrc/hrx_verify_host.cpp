// hrx_verify_host.cpp — the host form of VERIFY (include/hrx.h hrx_verify_rows_host): the rules of hrx_verify.hpp over rows in host memory, string-major
// (tight or pitched) or position-major as copied from the device, over threads by ranges of strings.  No HIP, no allocation; the host twin of
// hrx_kernel_verify.hip and the definition of the verdict word's row field.  tests/host_cpp/test_verify_host.cpp includes this file as it is.
// verify_rows_chunked_host is the host form of the chunked rule (hrx_verify_rows_chunked_host): threads over (string, chunk) pairs, then the fold per string.
#include "hrx_over_threads.hpp"
#include "hrx_verify.hpp"

namespace hrx {

// arguments checked by the caller (a.image: build_verify_image of the config, in host memory).  threads: 0 = as many as the machine has, at most 16;
// never more than one per 64 strings
void verify_rows_host(const VerifyArgs &a, unsigned threads) {
    if (a.B == 0 || a.M == 0) return;
    with_rows_form(a, [&a, threads](auto form) {
        over_threads(a.B, (unsigned)std::min<size_t>(rows_host_threads(threads), ((size_t)a.B + 63) / 64), [&a](size_t b0, size_t b1) {
            for (size_t b = b0; b < b1; ++b) a.verdict[b] = verify_string(a.image, a.D, a.lens[b], a.M, RowsOf<decltype(form)::value>(a, b));
        });
    });
}

// The chunked rule on the host (hrx_verify_rows_chunked_host): verify_chunk_string over (string, chunk) pairs — so a few long strings still use every
// thread — into summaries laid out as the kernel's ([field][chunk][string]), then verify_fold_chunk per string.  `summaries`: [kVfyChunkFields][K][B] u32.
// chunk_rows: a multiple of kVfyChunkAlign.
void verify_rows_chunked_host(const VerifyArgs &a, uint32_t chunk_rows, uint32_t *summaries, unsigned threads) {
    if (a.B == 0 || a.M == 0) return;
    threads = rows_host_threads(threads);
    const size_t B = a.B, K = verify_chunk_count(a.M, chunk_rows);
    with_rows_form(a, [&a, chunk_rows, summaries, B, K, threads](auto form) {
    over_threads(B * K, threads, [&a, chunk_rows, summaries, B, K](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            const size_t b = i / K, k = i % K;
            if (a.lens[b] > a.M) continue;          // no rows: no chunk of the string reads one
            const uint32_t r0 = (uint32_t)k * chunk_rows, r1 = (uint32_t)std::min<size_t>(a.M, (size_t)r0 + chunk_rows);
            const VerifyChunk v = verify_chunk_string(a.image, a.D, a.lens[b], a.M, r0, r1, RowsOf<decltype(form)::value>(a, b));
            const uint32_t w[kVfyChunkFields] = {v.flags, v.row, v.mask_row[0], v.mask_row[1], v.need1[0], v.need1[1], v.need0[0], v.need0[1]};
            for (size_t f = 0; f < kVfyChunkFields; ++f) summaries[(f * K + k) * B + b] = w[f];
        }
    });
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
