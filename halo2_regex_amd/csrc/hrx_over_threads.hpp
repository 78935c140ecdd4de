// hrx_over_threads.hpp — the host readers' split over threads (hrx_verify_host.cpp, hrx_lookup_host.cpp).  Host only: no kernel file includes it.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <thread>
#include <vector>

namespace hrx {

// `threads` as the host entry points take it: 0 = as many as the machine has, at most 16 (a caller with one
// piece of work per string allows no more than one thread per 64 strings)
inline unsigned rows_host_threads(unsigned threads) { return threads ? threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency())); }
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

}  // namespace hrx
