// hrx_compress_host.cpp — the host forms of LOOKUP COMPRESS (include/hrx.h hrx_lookup_compress_inputs_host / hrx_lookup_compress_table_host):
// compress_string of hrx_compress.hpp over rows in host memory, string-major (tight or pitched) or position-major as copied from the device, over threads by
// ranges of strings; the table's tuples over threads by ranges of rows.  No HIP, no allocation; the host twins of hrx_kernel_compress.hip and the
// definition of the cells.  tests/host_cpp/test_compress_host.cpp includes this file as it is.
#include "hrx_compress.hpp"
#include "hrx_over_threads.hpp"

namespace hrx {

// arguments checked by the caller.  threads: 0 = as many as the machine has, at most 16; never more than one per 64 strings
void compress_inputs_host(const CompressArgs &a, unsigned threads) {
    if (a.b_count == 0 || a.M == 0) return;
    with_rows_form(a, [&a, threads](auto form) {
        over_threads(a.b_count, (unsigned)std::min<size_t>(rows_host_threads(threads), ((size_t)a.b_count + 63) / 64), [&a](size_t i0, size_t i1) {
            FrPowers p;
            for (size_t i = i0; i < i1; ++i) {      // strings [i0, i1) of the window
                const size_t b = (size_t)a.b_begin + i;
                if (i == i0 || a.theta_stride) p = fr_powers(a.theta + i * a.theta_stride, a.canonical != 0);
                compress_string(a, i, a.lens[b], RowsOf<decltype(form)::value>(a, b), p);
            }
        });
    });
}

// ... never more than one thread per 1024 cells
void compress_table_host(const CompressTableArgs &a, unsigned threads) {
    const size_t cells = (size_t)a.n_theta * a.W;
    if (cells == 0) return;
    over_threads(cells, (unsigned)std::min<size_t>(rows_host_threads(threads), (cells + 1023) / 1024), [&a](size_t c0, size_t c1) {
        FrPowers p;
        size_t run = (size_t)-1;
        for (size_t c = c0; c < c1; ++c) {
            const size_t t = c / a.W, w = c - t * a.W;
            if (t != run) {
                p = fr_powers(a.theta + t * a.theta_stride, a.canonical != 0);
                run = t;
            }
            const uint32_t *tup = a.image + 4 * w;
            fr_store_cell(a.cells + 4 * c, fr_fold(tup[0], tup[1], tup[2], tup[3], p));
        }
    });
}

}  // namespace hrx
