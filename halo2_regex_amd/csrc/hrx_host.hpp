// hrx_host.hpp — C++ host-side mirror of the reference's Rust surface for the path, over the C ABI (include/hrx.h).
// Header only.  Same names, argument meaning and error behaviour as src/defs.rs and src/lib.rs:
//   AllstrRegexDef::read_from_text / SubstrRegexDef::read_from_text / ::new     defs.rs:54, 184, 147
//   RegexVerifyConfig::configure / load / derive_states / derive_substr_ids /
//     derive_is_start_end / match_substrs                                       lib.rs:126, 779, 804, 825, 847, 311
// Where the reference panics (parse errors, lib.rs:817) these throw std::runtime_error with the same text.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hrx.h"

namespace hrx_host {

inline void check(int rc) {
    if (rc != HRX_OK) throw std::runtime_error(hrx_last_error());
}

struct AllstrRegexDef {  // defs.rs:26-36 (parsed inside the library)
    std::string text, path;
    static AllstrRegexDef read_from_text(const std::string &file_path) { AllstrRegexDef d; d.path = file_path; return d; }
    static AllstrRegexDef from_string(std::string t) { AllstrRegexDef d; d.text = std::move(t); return d; }
};

struct SubstrRegexDef {  // defs.rs:115-132
    std::string text, path;
    std::vector<std::pair<uint64_t, uint64_t>> valid_state_transitions;
    std::vector<uint64_t> start_states, end_states;
    bool structured = false;
    static SubstrRegexDef read_from_text(const std::string &file_path) { SubstrRegexDef d; d.path = file_path; return d; }
    static SubstrRegexDef from_string(std::string t) { SubstrRegexDef d; d.text = std::move(t); return d; }
    // SubstrRegexDef::new (defs.rs:147-163); max_length/min_position/max_position are unused by the chip
    static SubstrRegexDef new_(size_t, uint64_t, uint64_t, std::vector<std::pair<uint64_t, uint64_t>> transitions,
                               std::vector<uint64_t> starts, std::vector<uint64_t> ends) {
        SubstrRegexDef d;
        d.structured = true;
        d.valid_state_transitions = std::move(transitions);
        d.start_states = std::move(starts);
        d.end_states = std::move(ends);
        return d;
    }
};

struct RegexDefs {  // defs.rs:17-22
    AllstrRegexDef allstr;
    std::vector<SubstrRegexDef> substrs;
};

// AssignedRegexResult (lib.rs:79-93), integers instead of assigned cells
struct AssignedRegexResult {
    std::vector<uint64_t> all_enable_flags, all_characters, all_substr_ids, masked_characters;
    std::vector<std::vector<uint64_t>> states, substr_ids, start_enables, end_enables;  // [def][row]
    uint64_t status = 0;
};

class RegexVerifyConfig {
   public:
    std::vector<RegexDefs> regex_defs;  // pub field, lib.rs:112

    // configure(meta, max_chars_size, gate, regex_defs) minus the halo2 objects (lib.rs:126-131)
    static RegexVerifyConfig configure(size_t max_chars_size, std::vector<RegexDefs> defs, int device = 0) {
        RegexVerifyConfig c;
        c.max_chars_size_ = max_chars_size;
        c.regex_defs = std::move(defs);
        check(hrx_defs_create(&c.defs_));
        for (const RegexDefs &rd : c.regex_defs) {
            if (!rd.allstr.path.empty()) check(hrx_defs_push_allstr_file(c.defs_, rd.allstr.path.c_str()));
            else check(hrx_defs_push_allstr_text(c.defs_, rd.allstr.text.data(), rd.allstr.text.size()));
            for (const SubstrRegexDef &sd : rd.substrs) {
                if (sd.structured) {
                    std::vector<uint64_t> a, b;
                    for (auto &p : sd.valid_state_transitions) { a.push_back(p.first); b.push_back(p.second); }
                    check(hrx_defs_push_substr(c.defs_, a.size(), a.data(), b.data(), sd.start_states.size(), sd.start_states.data(),
                                               sd.end_states.size(), sd.end_states.data()));
                } else if (!sd.path.empty()) check(hrx_defs_push_substr_file(c.defs_, sd.path.c_str()));
                else check(hrx_defs_push_substr_text(c.defs_, sd.text.data(), sd.text.size()));
            }
        }
        check(hrx_defs_finalize(c.defs_));
        if (device >= 0) check(hrx_ctx_create(c.defs_, device, &c.ctx_));
        return c;
    }
    RegexVerifyConfig() = default;
    RegexVerifyConfig(RegexVerifyConfig &&o) noexcept { *this = std::move(o); }
    RegexVerifyConfig &operator=(RegexVerifyConfig &&o) noexcept {
        std::swap(defs_, o.defs_); std::swap(ctx_, o.ctx_); std::swap(max_chars_size_, o.max_chars_size_);
        regex_defs = std::move(o.regex_defs);
        return *this;
    }
    RegexVerifyConfig(const RegexVerifyConfig &) = delete;
    ~RegexVerifyConfig() { if (ctx_) hrx_ctx_destroy(ctx_); if (defs_) hrx_defs_destroy(defs_); }

    size_t num_defs() const { return hrx_defs_num_defs(defs_); }
    hrx_ctx *ctx() const { return ctx_; }

    // load (lib.rs:779-785): the integer rows RegexTableConfig::load assigns, per def
    std::vector<std::vector<uint64_t>> load_transition_rows() const {
        std::vector<std::vector<uint64_t>> out;
        for (size_t d = 0; d < num_defs(); ++d) {
            std::vector<uint64_t> r(4 * hrx_table_transition_rows(defs_, d, nullptr, 0));
            hrx_table_transition_rows(defs_, d, r.data(), r.size() / 4);
            out.push_back(std::move(r));
        }
        return out;
    }

    std::vector<std::vector<uint64_t>> derive_states(const std::vector<uint8_t> &characters) const {  // lib.rs:804
        const size_t n = characters.size(), D = num_defs();
        std::vector<uint64_t> flat(D * (n + 1));
        check(hrx_derive_states(ctx_, characters.data(), n, flat.data()));
        return split(flat, D, n + 1);
    }
    std::vector<std::vector<uint64_t>> derive_substr_ids(const std::vector<std::vector<uint64_t>> &states) const {  // lib.rs:825
        const size_t D = states.size(), n = states[0].size() - 1;
        std::vector<uint64_t> out(D * n);
        check(hrx_derive_substr_ids(ctx_, join(states).data(), n, out.data()));
        return split(out, D, n);
    }
    std::pair<std::vector<std::vector<uint8_t>>, std::vector<std::vector<uint8_t>>> derive_is_start_end(
        const std::vector<std::vector<uint64_t>> &states, const std::vector<std::vector<uint64_t>> &substr_ids) const {  // lib.rs:847
        const size_t D = states.size(), n = states[0].size() - 1;
        std::vector<uint8_t> st(D * (n + 1)), en(D * (n + 1));
        check(hrx_derive_is_start_end(ctx_, join(states).data(), join(substr_ids).data(), n, st.data(), en.data()));
        std::vector<std::vector<uint8_t>> a(D), b(D);
        for (size_t d = 0; d < D; ++d) {
            a[d].assign(st.begin() + d * (n + 1), st.begin() + (d + 1) * (n + 1));
            b[d].assign(en.begin() + d * (n + 1), en.begin() + (d + 1) * (n + 1));
        }
        return {a, b};
    }
    AssignedRegexResult match_substrs(const std::vector<uint8_t> &characters) const {  // lib.rs:311
        const size_t M = max_chars_size_, D = num_defs();
        AssignedRegexResult r;
        r.all_enable_flags.resize(M); r.all_characters.resize(M); r.all_substr_ids.resize(M); r.masked_characters.resize(M);
        std::vector<uint64_t> st(D * M), sid(D * M), se(D * M), ee(D * M);
        check(hrx_match_substrs(ctx_, characters.data(), characters.size(), M, r.all_enable_flags.data(), r.all_characters.data(),
                                st.data(), sid.data(), se.data(), ee.data(), r.masked_characters.data(), r.all_substr_ids.data(),
                                &r.status));
        r.states = split(st, D, M); r.substr_ids = split(sid, D, M); r.start_enables = split(se, D, M); r.end_enables = split(ee, D, M);
        return r;
    }

    // EXTRACT (include/hrx.h): the revealed bytes of a list of strings as a list column, on the host: the ragged host match, then hrx_extract_spans_host
    struct Extracted {
        std::vector<uint64_t> status, run_offsets, runs, byte_offsets;
        std::vector<uint8_t> values;
    };
    Extracted extract_strings(const std::vector<std::vector<uint8_t>> &strings, size_t max_spans = 16, uint32_t require_accept = 0) const {
        const size_t B = strings.size();
        std::vector<uint64_t> offsets(B + 1, 0);
        std::vector<uint8_t> bytes;
        for (size_t b = 0; b < B; ++b) {
            bytes.insert(bytes.end(), strings[b].begin(), strings[b].end());
            offsets[b + 1] = bytes.size();
        }
        bytes.resize(bytes.size() + 16);
        Extracted e;
        e.status.resize(B);
        std::vector<uint32_t> counts(B + 2);
        std::vector<uint64_t> spans(B * max_spans + 1), totals(4);
        check(hrx_match_batch_host_ragged(ctx_, bytes.data(), offsets.data(), B, max_chars_size_, e.status.data(), counts.data(), spans.data(), max_spans));
        e.run_offsets.resize(B + 1); e.runs.resize(B * max_spans); e.byte_offsets.resize(B * max_spans + 1); e.values.resize(bytes.size());
        const hrx_extract_out out{e.run_offsets.data(), e.runs.data(), e.byte_offsets.data(), e.values.data(), totals.data(), e.runs.size(), e.values.size()};
        check(hrx_extract_spans_host(HRX_LAYOUT_INPUT_RAGGED, bytes.data(), 0, offsets.data(), B, e.status.data(), counts.data(), spans.data(), max_spans,
                                     require_accept, &out, 0));
        e.runs.resize(totals[0]); e.byte_offsets.resize(totals[0] + 1); e.values.resize(totals[1]);
        return e;
    }
    // ... and the device form as it is (device pointers; `workspace` of hrx_extract_workspace_bytes(B) bytes; asynchronous on `stream`)
    static size_t extract_workspace_bytes(size_t B) { return hrx_extract_workspace_bytes(B); }
    void extract_spans_device(int layout, const uint8_t *src, size_t stride, const uint64_t *offsets, size_t B, const uint64_t *status, const uint32_t *span_counts,
                              const uint64_t *spans, size_t max_spans, uint32_t require_accept, const hrx_extract_out &out, void *workspace, size_t workspace_bytes,
                              void *stream) const {
        check(hrx_extract_spans_device(ctx_, layout, src, stride, offsets, B, status, span_counts, spans, max_spans, require_accept, &out, workspace, workspace_bytes, stream));
    }

    // VERIFY (include/hrx.h): one verdict word per string for rows in host memory (string-major with pitches in rows, 0 = M; or position-major), and the device
    // forms as they are (device pointers, asynchronous on `stream`)
    std::vector<uint64_t> verify_rows_host(int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                                           const uint16_t *masked, size_t msk_pitch, size_t B) const {
        std::vector<uint64_t> verdict(B);
        check(hrx_verify_rows_host(ctx_, layout, chars, stride, lens, records, rec_pitch, masked, msk_pitch, B, max_chars_size_, verdict.data()));
        return verdict;
    }
    void verify_rows_device(int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch, const uint16_t *masked,
                            size_t msk_pitch, size_t B, uint64_t *verdict, void *stream) const {
        check(hrx_verify_rows_device(ctx_, layout, chars, stride, lens, records, rec_pitch, masked, msk_pitch, B, max_chars_size_, verdict, stream));
    }
    void verify_rows_device_planes(int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *const *record_planes, size_t n_planes,
                                   const uint16_t *masked, size_t B, uint64_t *verdict, void *stream) const {
        check(hrx_verify_rows_device_planes(ctx_, layout, chars, stride, lens, record_planes, n_planes, masked, B, max_chars_size_, verdict, stream));
    }

    // LOOKUP PRODUCT (include/hrx.h): the inverse tables 1 / (S + shift) of compressed table runs and the grand product Z, as the C calls are (device pointers
    // and `stream` for the device forms, host memory for the host forms); flags: 0 or HRX_FR_CANONICAL
    static size_t lookup_invert_workspace_bytes(const hrx_defs *defs, size_t n_runs) { return hrx_lookup_invert_workspace_bytes(defs, n_runs); }
    void lookup_invert_table_device(const uint64_t *table_cells, size_t n_runs, const uint64_t *shift, size_t shift_stride, uint64_t *inv_cells, int flags,
                                    void *workspace, size_t workspace_bytes, void *stream) const {
        check(hrx_lookup_invert_table_device(ctx_, table_cells, n_runs, shift, shift_stride, inv_cells, flags, workspace, workspace_bytes, stream));
    }
    void lookup_invert_table_host(const uint64_t *table_cells, size_t n_runs, const uint64_t *shift, size_t shift_stride, uint64_t *inv_cells, int flags) const {
        check(hrx_lookup_invert_table_host(ctx_, table_cells, n_runs, shift, shift_stride, inv_cells, flags));
    }
    void lookup_product_device(const uint32_t *lens, size_t b_begin, size_t b_count, const uint64_t *in_cells, const uint32_t *a_idx, const uint32_t *s_idx,
                               size_t n_rows, size_t idx_pitch, const uint64_t *table_cells, const uint64_t *inv_beta, const uint64_t *inv_gamma, size_t table_stride,
                               const uint64_t *beta, const uint64_t *gamma, size_t challenge_stride, uint64_t *z, size_t z_pitch, uint32_t *open, int flags,
                               void *stream) const {
        check(hrx_lookup_product_device(ctx_, lens, max_chars_size_, b_begin, b_count, in_cells, a_idx, s_idx, n_rows, idx_pitch, table_cells, inv_beta, inv_gamma,
                                        table_stride, beta, gamma, challenge_stride, z, z_pitch, open, flags, stream));
    }
    void lookup_product_host(const uint32_t *lens, size_t b_begin, size_t b_count, const uint64_t *in_cells, const uint32_t *a_idx, const uint32_t *s_idx,
                             size_t n_rows, size_t idx_pitch, const uint64_t *table_cells, const uint64_t *inv_beta, const uint64_t *inv_gamma, size_t table_stride,
                             const uint64_t *beta, const uint64_t *gamma, size_t challenge_stride, uint64_t *z, size_t z_pitch, uint32_t *open, int flags) const {
        check(hrx_lookup_product_host(ctx_, lens, max_chars_size_, b_begin, b_count, in_cells, a_idx, s_idx, n_rows, idx_pitch, table_cells, inv_beta, inv_gamma,
                                      table_stride, beta, gamma, challenge_stride, z, z_pitch, open, flags));
    }
    void lookup_product_plan(size_t b_count, size_t n_rows, size_t *tile_rows, size_t *rows_per_lane) const {
        check(hrx_ctx_lookup_product_plan(ctx_, b_count, n_rows, tile_rows, rows_per_lane));
    }

    // FR NTT (include/hrx.h): the transform of size 2^k over columns of field cells, as the C calls are; flags: HRX_FR_CANONICAL | HRX_NTT_INVERSE
    static size_t fr_ntt_workspace_bytes(unsigned k) { return hrx_fr_ntt_workspace_bytes(k); }
    void fr_ntt_prepare_device(unsigned k, void *workspace, size_t workspace_bytes, void *stream) const {
        check(hrx_fr_ntt_prepare_device(ctx_, k, workspace, workspace_bytes, stream));
    }
    void fr_ntt_device(const uint64_t *in, size_t in_pitch, uint64_t *out, size_t out_pitch, size_t n_cols, unsigned k, size_t n_in, const uint64_t *shift, int flags,
                       const void *workspace, size_t workspace_bytes, void *stream) const {
        check(hrx_fr_ntt_device(ctx_, in, in_pitch, out, out_pitch, n_cols, k, n_in, shift, flags, workspace, workspace_bytes, stream));
    }
    void fr_ntt_host(const uint64_t *in, size_t in_pitch, uint64_t *out, size_t out_pitch, size_t n_cols, unsigned k, size_t n_in, const uint64_t *shift,
                     int flags) const {
        check(hrx_fr_ntt_host(ctx_, in, in_pitch, out, out_pitch, n_cols, k, n_in, shift, flags));
    }

    // LOOKUP QUOTIENT (include/hrx.h): the lookup argument's five constraints on the extended coset, as the C calls are; flags: HRX_FR_CANONICAL |
    // HRX_QUOTIENT_DIVIDE
    void fr_vanishing_inverse_device(unsigned k, unsigned ext_k, const uint64_t *shift, uint64_t *t_inv, int flags, void *stream) const {
        check(hrx_fr_vanishing_inverse_device(ctx_, k, ext_k, shift, t_inv, flags, stream));
    }
    void fr_vanishing_inverse_host(unsigned k, unsigned ext_k, const uint64_t *shift, uint64_t *t_inv, int flags) const {
        check(hrx_fr_vanishing_inverse_host(ctx_, k, ext_k, shift, t_inv, flags));
    }
    void lookup_quotient_device(size_t b_count, unsigned k, unsigned ext_k, const uint64_t *a_ext, const uint64_t *ap_ext, const uint64_t *sp_ext,
                                const uint64_t *z_ext, size_t pitch, const uint64_t *s_ext, size_t s_pitch, size_t s_stride, const uint64_t *selectors,
                                size_t sel_pitch, const uint64_t *beta, const uint64_t *gamma, const uint64_t *y, size_t challenge_stride, const uint64_t *h_in,
                                uint64_t *h_out, size_t h_pitch, const uint64_t *t_inv, int flags, void *stream) const {
        check(hrx_lookup_quotient_device(ctx_, b_count, k, ext_k, a_ext, ap_ext, sp_ext, z_ext, pitch, s_ext, s_pitch, s_stride, selectors, sel_pitch, beta, gamma, y,
                                         challenge_stride, h_in, h_out, h_pitch, t_inv, flags, stream));
    }
    void lookup_quotient_host(size_t b_count, unsigned k, unsigned ext_k, const uint64_t *a_ext, const uint64_t *ap_ext, const uint64_t *sp_ext,
                              const uint64_t *z_ext, size_t pitch, const uint64_t *s_ext, size_t s_pitch, size_t s_stride, const uint64_t *selectors,
                              size_t sel_pitch, const uint64_t *beta, const uint64_t *gamma, const uint64_t *y, size_t challenge_stride, const uint64_t *h_in,
                              uint64_t *h_out, size_t h_pitch, const uint64_t *t_inv, int flags) const {
        check(hrx_lookup_quotient_host(ctx_, b_count, k, ext_k, a_ext, ap_ext, sp_ext, z_ext, pitch, s_ext, s_pitch, s_stride, selectors, sel_pitch, beta, gamma, y,
                                       challenge_stride, h_in, h_out, h_pitch, t_inv, flags));
    }
    void lookup_quotient_plan(size_t b_count, unsigned ext_k, size_t *tile_cells, size_t *cells_per_lane) const {
        check(hrx_ctx_lookup_quotient_plan(ctx_, b_count, ext_k, tile_cells, cells_per_lane));
    }

   private:
    static std::vector<std::vector<uint64_t>> split(const std::vector<uint64_t> &f, size_t D, size_t len) {
        std::vector<std::vector<uint64_t>> o(D);
        for (size_t d = 0; d < D; ++d) o[d].assign(f.begin() + d * len, f.begin() + (d + 1) * len);
        return o;
    }
    static std::vector<uint64_t> join(const std::vector<std::vector<uint64_t>> &v) {
        std::vector<uint64_t> o;
        for (auto &x : v) o.insert(o.end(), x.begin(), x.end());
        return o;
    }
    hrx_defs *defs_ = nullptr;
    hrx_ctx *ctx_ = nullptr;
    size_t max_chars_size_ = 0;
};

}  // namespace hrx_host
