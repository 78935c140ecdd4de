// hrx_lookup_host.cpp — the host form of LOOKUP COUNTS (include/hrx.h hrx_lookup_counts_host): lookup_string of hrx_lookup.hpp over rows in host memory,
// string-major (tight or pitched) or position-major as copied from the device, over threads by ranges of strings.  No HIP, no allocation; the host twin of
// hrx_kernel_lookup.hip and the definition of the counts.  tests/host_cpp/test_lookup_host.cpp includes this file as it is.
#include "hrx_lookup.hpp"
#include "hrx_over_threads.hpp"

namespace hrx {

// arguments checked by the caller (a.image: build_lookup_image of the config, in host memory; a.W its lookup_words).  threads: 0 = as many as the machine
// has, at most 16; never more than one per 64 strings
void lookup_counts_host(const LookupArgs &a, unsigned threads) {
    if (a.b_count == 0 || a.M == 0) return;
    with_rows_form(a, [&a, threads](auto form) {
        over_threads(a.b_count, (unsigned)std::min<size_t>(rows_host_threads(threads), ((size_t)a.b_count + 63) / 64), [&a](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; ++i) {      // strings [i0, i1) of the window
                const size_t b = (size_t)a.b_begin + i;
                const uint32_t m = lookup_string(a.image, a.D, a.lens[b], a.M, RowsOf<decltype(form)::value>(a, b), a.counts + i * a.W);
                if (a.misses) a.misses[i] = m;
            }
        });
    });
}

}  // namespace hrx
