// hrx_rows.hpp — the ROW FORMS, once: what a reader of witness rows is told (RowsIn) and where a cell of string b lies (RowsPlace), for every form
// include/hrx.h defines — records string-major (tight or pitched), position-major interleaved, record planes, the two row stripes of one def; the input
// bytes string-major or position-major; position-major buffers blocked by HRX_PM_BLOCK strings.  No HIP dependency: the kernels that read rows
// (hrx_kernel_verify.hip, hrx_kernel_lookup.hip, fr_columns_kernel of hrx_kernel.hip), the host readers (hrx_verify_host.cpp, hrx_lookup_host.cpp,
// hrx_fill.cpp, the hrx_rows_of_string_* of hrx_api.cpp) and tests/host_cpp/test_rows_host.cpp all include it.  The writers of rows (the witness
// kernels) have their own storers.  DESIGN.md §19.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/hrx.h"

#ifndef HRX_XHD
#if defined(__HIP__)  // clang in HIP mode (hipcc), host and device passes alike
#define HRX_XHD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define HRX_XHD inline
#endif
#endif

namespace hrx {

constexpr uint32_t kRowsMaxPlanes = 8;              // record buffers of one launch (hrx_kernel.hpp kMaxDefsPerLaunch: the status word's accept bits)
constexpr uint32_t kRowsMaxRows = 1u << 24;         // the largest M a witness entry point takes

// What a reader of rows is told.  The readers' own argument structs (VerifyArgs, LookupArgs, FrArgs) derive from it.
struct RowsIn {
    const uint8_t *chars;
    uint64_t stride;
    const uint32_t *lens;
    const uint32_t *records;                        // interleaved records (string-major or position-major), or NULL: planes
    const uint16_t *masked;                         // NULL: the reader has no masked rows
    const uint32_t *planes[kRowsMaxPlanes];         // record planes, or the two row stripes of one def
    uint32_t n_stripes;                             // 2: planes[] are the row stripes of one def
    uint32_t B, M, D, layout;
    uint64_t rec_pitch, msk_pitch;                  // string-major: rows between consecutive strings
};

// A caller's rows as an entry point receives them, before any check: what check_rows (hrx_rows_api.cpp) makes a RowsIn of.  records or planes / n_planes,
// the other NULL / 0; masked NULL and msk_pitch 0 where the reader has no masked rows; a pitch of 0: M
struct RowsCall {
    int layout;
    const uint8_t *chars;
    size_t stride;
    const uint32_t *lens, *records;
    const uint32_t *const *planes;
    size_t n_planes, rec_pitch;
    const uint16_t *masked;
    size_t msk_pitch, B, M;
};

// the record form: a template parameter of the kernels, a run-time value (rows_form) of the host readers
enum : int { kRecSm = 0, kRecPm = 1, kRecPlanes = 2 };
HRX_XHD int rows_form(const RowsIn &a) { return !(a.layout & HRX_LAYOUT_POSITION_MAJOR) ? kRecSm : a.records ? kRecPm : kRecPlanes; }
// the layouts a reader of rows takes
HRX_XHD bool rows_layout_known(int layout) {
    return layout == HRX_LAYOUT_STRING_MAJOR || layout == HRX_LAYOUT_POSITION_MAJOR || layout == (HRX_LAYOUT_POSITION_MAJOR | HRX_LAYOUT_INPUT_POSITION_MAJOR);
}

// where string b's cells lie
struct RowsPlace {
    const unsigned char *chr;   // byte i at chr + (i / 16) * chr_step + i % 16
    size_t chr_step;
    const uint16_t *msk;        // position-major: octet o at msk + o * msk_step; string-major: row r at msk + r; NULL: no masked rows
    size_t msk_step;
    const uint32_t *rec;        // position-major: quad q of def d at rec + (q * D + d) * rec_step; string-major: (r, d) at rec + r * D + d
    size_t rec_step;            // planes: quad q at plane[(q % R) * D + d] + pl_off + (q / R) * rec_step
    size_t pl_off;
};

// MSK: the reader has masked rows (a.masked is not NULL).  Without them no address is formed from a.masked, and none is tested for it where it is there
template <bool MSK>
HRX_XHD RowsPlace rows_place(const RowsIn &a, const uint32_t b) {
    RowsPlace s;
    const bool pm = (a.layout & HRX_LAYOUT_POSITION_MAJOR) != 0, in_pm = (a.layout & HRX_LAYOUT_INPUT_POSITION_MAJOR) != 0;
    constexpr uint32_t kBlock = HRX_PM_BLOCK;
    const uint32_t blk0 = (b / kBlock) * kBlock, left = a.B - blk0, nb = left < kBlock ? left : kBlock, bl = b - blk0;
    const size_t q4 = (a.M + 3u) / 4u, q8 = (a.M + 7u) / 8u;
    if (in_pm) {
        s.chr = a.chars + (size_t)blk0 * a.stride + (size_t)bl * 16u;
        s.chr_step = (size_t)nb * 16u;
    } else {
        s.chr = a.chars + (size_t)b * a.stride;
        s.chr_step = 16u;
    }
    if (pm) {
        if constexpr (MSK) s.msk = a.masked + ((size_t)blk0 * q8 + bl) * 8u;
        else s.msk = nullptr;
        s.msk_step = (size_t)nb * 8u;
        s.rec = a.records ? a.records + ((size_t)blk0 * q4 * a.D + bl) * 4u : nullptr;
        s.rec_step = (size_t)nb * 4u;
        const size_t R = a.n_stripes == 2u ? 2u : 1u;
        s.pl_off = ((size_t)blk0 * ((q4 + R - 1u) / R) + bl) * 4u;
    } else {
        if constexpr (MSK) s.msk = a.masked + (size_t)b * a.msk_pitch;
        else s.msk = nullptr;
        s.msk_step = 0;
        s.rec = a.records + (size_t)b * a.rec_pitch * a.D;
        s.rec_step = 0;
        s.pl_off = 0;
    }
    return s;
}

// ---- the addresses of the kernels' vector loads
// the 16-byte input chunk that holds byte i
HRX_XHD const unsigned char *chr_chunk(const RowsPlace &s, const uint32_t i) { return s.chr + (size_t)(i >> 4) * s.chr_step; }
// masked octet o: rows 8 o .. 8 o + 7, 16 bytes (position-major)
HRX_XHD const uint16_t *msk_octet(const RowsPlace &s, const uint32_t o) { return s.msk + (size_t)o * s.msk_step; }
// def d's record quad q: rows 4 q .. 4 q + 3, 16 bytes (REC: kRecPm or kRecPlanes)
template <int REC>
HRX_XHD const uint32_t *rec_quad(const RowsIn &a, const RowsPlace &s, const uint32_t q, const uint32_t d) {
    static_assert(REC == kRecPm || REC == kRecPlanes, "string-major records have no quads");
    if constexpr (REC == kRecPm) {
        return s.rec + ((size_t)q * a.D + d) * s.rec_step;
    } else {
        const uint32_t R = a.n_stripes == 2u ? 2u : 1u;
        return a.planes[(q % R) * a.D + d] + s.pl_off + (size_t)(q / R) * s.rec_step;
    }
}

// ---- single cells
HRX_XHD uint32_t chr_cell(const RowsPlace &s, const uint32_t i) { return chr_chunk(s, i)[i & 15u]; }
template <bool PM>
HRX_XHD uint32_t msk_cell(const RowsPlace &s, const uint32_t r) {
    if constexpr (PM) return msk_octet(s, r >> 3)[r & 7u];
    else return s.msk[r];
}
template <int REC>
HRX_XHD uint32_t rec_cell(const RowsIn &a, const RowsPlace &s, const uint32_t r, const uint32_t d) {
    if constexpr (REC == kRecSm) return s.rec[(size_t)r * a.D + d];
    else return rec_quad<REC>(a, s, r >> 2, d)[r & 3u];
}

// String b of rows of form REC: the accessor verify_string / lookup_string walk over, and what every host reader reads through.  with_rows_form
// takes the form of `a` at run time, once per call: fn(form) with decltype(form)::value == kRecSm / kRecPm / kRecPlanes
template <int REC>
struct RowsOf {
    const RowsIn &a;
    RowsPlace s;
    RowsOf(const RowsIn &args, size_t b) : a(args), s(args.masked ? rows_place<true>(args, (uint32_t)b) : rows_place<false>(args, (uint32_t)b)) {}
    uint32_t chr(size_t i) const { return chr_cell(s, (uint32_t)i); }
    uint32_t rec(size_t r, size_t d) const { return rec_cell<REC>(a, s, (uint32_t)r, (uint32_t)d); }
    uint32_t msk(size_t r) const { return msk_cell<REC != kRecSm>(s, (uint32_t)r); }
};
template <class Fn>
inline void with_rows_form(const RowsIn &a, const Fn &fn) {
    switch (rows_form(a)) {
        case kRecSm: fn(std::integral_constant<int, kRecSm>{}); break;
        case kRecPm: fn(std::integral_constant<int, kRecPm>{}); break;
        default: fn(std::integral_constant<int, kRecPlanes>{}); break;
    }
}

}  // namespace hrx
