// hrx_verify_host.cpp — the host form of VERIFY (include/hrx.h hrx_verify_rows_host): the rules of hrx_verify.hpp over rows in host memory, string-major
// (tight or pitched) or position-major as copied from the device, over threads by ranges of strings.  No HIP, no allocation; the host twin of
// hrx_kernel_verify.hip and the definition of the verdict word's row field.  tests/host_cpp/test_verify_host.cpp includes this file as it is.
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

}  // namespace hrx
