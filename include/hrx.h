/*
 * hrx.h — C ABI of the MI355X-native batched DFA witness generator for halo2-regex.
 *
 * The reference (zkemail/halo2-regex) has no FFI: the seam this library replaces is
 * Rust-internal — the three pub(crate) methods RegexVerifyConfig::derive_states /
 * derive_substr_ids / derive_is_start_end (src/lib.rs:804-888) called at the top of
 * RegexVerifyConfig::match_substrs (src/lib.rs:316-318), the integer content of the
 * reveal-mask scan in match_substrs (src/lib.rs:593-764), the data model and text
 * parsers of src/defs.rs, and the fixed-table rows of RegexTableConfig::load
 * (src/table.rs:61-198).  Every entry point below cites the reference interface it
 * stands in for.  INTEGRATION.md shows the Rust binding a maintainer would add.
 *
 * Conventions: plain pointers and sizes, caller-owned buffers, integer status
 * returns (0 = HRX_OK), nothing unwinds.  Text of the last error: hrx_last_error().
 * Batches run on a gfx950 device: the device-pointer entry points fail with HRX_ERR_HIP without one.  The library's one
 * host-side compute path is its native small-batch walk (the same lane algorithm on a host core): the reference-shaped
 * single-string entry points and host-buffer batches below the context's threshold take it — match_substrs hands over ONE
 * string per call (src/lib.rs:316-318) and a GPU launch cannot beat a host core on ~1000 rows.
 */
#ifndef HRX_H
#define HRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hrx_defs hrx_defs; /* Vec<RegexDefs> (src/defs.rs:17-22) + the dense fused tables built from it */
typedef struct hrx_ctx hrx_ctx;   /* one device: tables resident in HBM, a stream, staging buffers */

enum {
    HRX_OK = 0,
    HRX_ERR_PARSE = 1,              /* where AllstrRegexDef/SubstrRegexDef::read_from_reader panics (defs.rs:85-91, 219-225) */
    HRX_ERR_BOUNDS = 2,             /* state / substr-id ranges the compact record or the LDS table cannot hold */
    HRX_ERR_ARG = 3,
    HRX_ERR_HIP = 4,
    HRX_ERR_STATE = 5,              /* call order (e.g. push after finalize) */
    HRX_ERR_INVALID_TRANSITION = 6, /* single-string API: the reference's panic at src/lib.rs:817 */
    HRX_ERR_OUT_OF_CONTRACT = 7,    /* single-string API: two defs flag the same row or n > max_chars_size */
    HRX_ERR_IO = 8
};

/* ------------------------------------------------------------------ */
/* Data model — src/defs.rs                                            */
/* ------------------------------------------------------------------ */

int hrx_defs_create(hrx_defs **out);
void hrx_defs_destroy(hrx_defs *defs);

/* AllstrRegexDef::read_from_reader (defs.rs:75-110) on an in-memory text; begins a new
 * RegexDefs { allstr, substrs: vec![] }.  Line 0 first state, line 1 accepted state,
 * line 2 largest state, then "cur next char" per line; the char is taken `as u8`. */
int hrx_defs_push_allstr_text(hrx_defs *defs, const char *text, size_t len);
/* AllstrRegexDef::read_from_text (defs.rs:54-58) */
int hrx_defs_push_allstr_file(hrx_defs *defs, const char *path);
/* SubstrRegexDef::read_from_reader (defs.rs:209-265); appended to the last RegexDefs.substrs. */
int hrx_defs_push_substr_text(hrx_defs *defs, const char *text, size_t len);
/* SubstrRegexDef::read_from_text (defs.rs:184-188) */
int hrx_defs_push_substr_file(hrx_defs *defs, const char *path);
/* Already-parsed forms for a Rust caller that holds the structs:
 * AllstrRegexDef { state_lookup, first_state_val, accepted_state_val, largest_state_val } (defs.rs:26-36);
 * entry i is state_lookup[(chr[i], cur[i])] = (line_idx[i], next[i]). */
int hrx_defs_push_allstr(hrx_defs *defs, uint64_t first_state_val, uint64_t accepted_state_val,
                         uint64_t largest_state_val, size_t n_transitions, const uint64_t *cur,
                         const uint64_t *next, const uint8_t *chr, const uint64_t *line_idx);
/* SubstrRegexDef::new (defs.rs:147-163); max_length / min_position / max_position are unused by the chip. */
int hrx_defs_push_substr(hrx_defs *defs, size_t n_pairs, const uint64_t *pair_cur, const uint64_t *pair_next,
                         size_t n_start, const uint64_t *start_states, size_t n_end, const uint64_t *end_states);
/* Validate and build the dense fused (state,char) tables.  Required before any call below.
 * regex_defs is a Vec of any length in the reference (src/lib.rs:112; loops at :387, :806, :828, :855): up to HRX_MAX_DEFS
 * RegexDefs per config.  Up to three defs are walked side by side by one kernel launch; four to eight defs of at most 32 byte classes each (position-major
 * outputs) by ONE def-parallel launch — a walker wave per def over class-indexed tables, a combiner wave — at 0.66-0.70 of the HBM peak (nine defs and more: one such launch per group of up to eight defs + the combine launch, 0.58-0.65); a def of more than 32 byte classes puts its config into passes
 * over consecutive groups of defs (each group's tables LDS-resident); the per-row sums over all defs (reveal masks, flag
 * overlap) and the merged status are formed by the last pass itself from 80-byte tile summaries the earlier passes leave
 * (position-major outputs, up to four groups) or by a combine launch — same buffers, same results; with position-major outputs
 * the passes write the caller's record planes directly and the extra cost is ~2.5 bytes per row and earlier group.  String-major
 * outputs of more than three defs: four and five defs of at most 32 byte classes each, row counts in multiples of 16, come straight out of the
 * def-parallel launch (0.50-0.68 of peak: the records meet in LDS sub-tiles, a storer wave writes the caller's [B][pitch][D]); otherwise row counts
 * in multiples of 8 are produced position-major in context scratch and transposed (~0.2 of peak), and other row counts are copied into place by
 * the combine launch and are several times slower: ask for position-major buffers there.
 * HRX_MP_COMBINE=1 in the environment of hrx_ctx_create keeps the separate combine launch. */
#define HRX_MAX_DEFS 32
int hrx_defs_finalize(hrx_defs *defs);

size_t hrx_defs_num_defs(const hrx_defs *defs);
size_t hrx_defs_num_substrs(const hrx_defs *defs, size_t def);
uint64_t hrx_defs_first_state(const hrx_defs *defs, size_t def);
uint64_t hrx_defs_accepted_state(const hrx_defs *defs, size_t def);
uint64_t hrx_defs_largest_state(const hrx_defs *defs, size_t def);
size_t hrx_defs_num_transitions(const hrx_defs *defs, size_t def);
/* substr_id of the first substring of `def`: the offset rule of lib.rs:780-783 / 827,842 */
uint64_t hrx_defs_substr_id_offset(const hrx_defs *defs, size_t def);
/* bytes of LDS the fused tables of all defs occupy */
size_t hrx_defs_table_bytes(const hrx_defs *defs);

/* RegexTableConfig::load (table.rs:61-198), rows as integers in assignment order.
 * transition rows: (char, cur_state, next_state, substr_id), row 0 = (0,dummy,dummy,0), then one row per
 * state_lookup entry sorted by line index.  endpoint rows: (substr_id, start_state, end_state).
 * Returns the number of rows; writes min(rows, cap) of them. */
size_t hrx_table_transition_rows(const hrx_defs *defs, size_t def, uint64_t *rows4, size_t cap_rows);
size_t hrx_table_endpoint_rows(const hrx_defs *defs, size_t def, uint64_t *rows3, size_t cap_rows);

/* ------------------------------------------------------------------ */
/* Device context                                                      */
/* ------------------------------------------------------------------ */

int hrx_device_count(int *count);
/* Uploads the tables to `device` and creates a stream.  The handle may be shared by clones of a
 * RegexVerifyConfig (lib.rs:96 derives Clone); device work of one ctx is serialised internally.  A context owns device
 * scratch that some launches use (the group counter of multi-round batches, the group buffers of configs of more than three
 * defs): it serves ONE stream or captured graph at a time — a launch on another stream first waits on the host for the stream
 * that used the scratch last (HRX_ERR_STATE if that wait is impossible, e.g. inside a stream capture), and a captured graph
 * must not be replayed concurrently with other launches of the same context; use one context per concurrent stream.  Every entry point
 * leaves the caller's current HIP device as it found it.
 * device = HRX_DEVICE_NONE: a host-only context (no HIP call is made): the single-string entry points and
 * hrx_witness_batch_host run the native host walk, device-pointer entry points return HRX_ERR_HIP.
 * HRX_DEBUG_FLAGS (environment; kernel-selection bits for the tests, csrc/hrx_kernel.hpp) is read here, once. */
#define HRX_DEVICE_NONE (-1)
int hrx_ctx_create(const hrx_defs *defs, int device, hrx_ctx **out);
/* A second context of the same config: its own stream, scratch and lock, the same tables (uploaded again: ~100 KiB) and the source's per-context switches
 * (host threshold, placement).  RegexVerifyConfig derives Clone (src/lib.rs:96) and halo2 clones the config per synthesize pass / worker thread: a context
 * serves one stream at a time, so a prover that wants its threads to overlap gives every clone a context of its own (they share the device's measured arena pair,
 * hrx_alloc_output_pair).  device: a GPU index, HRX_DEVICE_NONE, or HRX_DEVICE_SAME (the source's).  The hrx_defs handle the source was made from need not exist any more. */
#define HRX_DEVICE_SAME (-2)
int hrx_ctx_clone(const hrx_ctx *ctx, int device, hrx_ctx **out);
void hrx_ctx_destroy(hrx_ctx *ctx);
int hrx_ctx_device(const hrx_ctx *ctx);
/* Host-buffer batches (hrx_witness_batch_host, hrx_multi_witness_batch_host) of fewer than `rows` witness rows (B x M)
 * are walked on the calling host thread instead of being staged to the device; default HRX_DEFAULT_HOST_THRESHOLD
 * (the measured crossover, NOTES_MEASUREMENTS.md §7c); 0 = always the device.  The single-string entry points below always take the
 * host walk (one GPU lane needs ~50 ns per row, a host core ~3).  Results are identical either way. */
#define HRX_DEFAULT_HOST_THRESHOLD 32768
int hrx_ctx_set_host_threshold(hrx_ctx *ctx, size_t rows);
size_t hrx_ctx_host_threshold(const hrx_ctx *ctx);
/* Per-context choices between variants that compute the same rows (what a linking prover sets instead of environment variables).
 *   HRX_OPT_PMD_COMBINER_WAVE  the def-parallel kernel of two- and three-def configs (batches of at most two groups of 64 strings per CU): 1 = a combiner wave of its own
 *                              per group (sums over the defs, reveal mask, masked rows), 2 = the last def's walker combines, 0 = the library's default
 *   HRX_OPT_HOST_ROUTE         hrx_witness_batch_host on a device context, batches of at least the host threshold:
 *                              HRX_HOST_ROUTE_AUTO (0, default) from 2^22 rows on the FASTEST OF THREE WAYS by this context's own measurements: everything through the device
 *                                (staged, walked, copied back: the copy back over the link bounds it, ~9e9 rows/s at one def), everything on the host cores (the native walk: the host's
 *                                cores and memory bound it), or both at once — the batch split by string index between them in the ratio of the two parts' rates.  The context's calls 0
 *                                and 1 go through the device (0 pays for allocations and is not recorded), 2 on the host cores, 3 and 4 split; from then on the way with the smallest time
 *                                per row, whose figure every call refreshes; every 32nd call re-measures one of the other two if its figure was within 1.5x of the best.  Smaller
 *                                batches: the device; below the host threshold: the host;
 *                              HRX_HOST_ROUTE_DEVICE (1) everything through the device;  HRX_HOST_ROUTE_HOST (2) everything on the host cores.  Results are identical either way.
 *   HRX_OPT_HOST_THREADS       host threads of the native walk (0, default: as many as the calling thread's affinity mask has cores; hrx_multi_create divides them among its shards)
 *   HRX_OPT_HOST_PIPELINE      the device part's transfers: 0 (default) the context times both ways over its first calls and keeps the faster (the pipeline's copies out run at half rate
 *                              on some hosts), 1 pipelined chunk by chunk over two streams, 2 in, walk, out on one stream; HRX_HOST_PIPELINE=1 / 0 in the environment of hrx_ctx_create
 *                              sets 1 / 2 as the context's default
 *   HRX_OPT_PLACE_DRY_LAUNCH   hrx_alloc_output_planes / _for_batch: 1 (default) the best candidate sets by the pairings' score are each launched into and the fastest is kept, 0 the best
 *                              by score is kept unlaunched (a profiler's kernel list then holds the caller's launches only)
 *   HRX_OPT_MATCH_FUSED_WIDE   the match entry points (MATCH, RAGGED, SELECTED below) on configs of four to eight RegexDefs: 0 (default) "via rows", 1 the fused walk — one lane
 *                              per string on the config's class-wide tables in LDS, no witness row written, no scratch, no slices — for string-major, ragged and selected input
 *                              where every def has at most 32 byte classes, the defs have at most 1023 table rows together and the tables fit LDS; every other config and
 *                              shape (position-major input, more than eight defs, HRX_DEBUG_FLAGS bit 32) stays via rows.  hrx_ctx_describe_match names what a shape takes.
 *                              Results are identical either way.  Recommended (measured at most 0.9 of the via-rows time, tools/match_wide_bench.py on 65536 x 1024 and 4 x 65536 x 1024) for
 *                              whole batches — string-major or ragged — whose strings mostly fill M (0.42 .. 0.60) or are mostly short with a few long (0.80 .. 0.89), and at four
 *                              defs for batches of several waves per SIMD (262144 strings: 0.70 .. 0.75).  NOT for a selection of a batch (the cascade: 0.92 .. 6.5 — a launch of
 *                              few strings lasts as long as its longest string's walk) nor for uniformly mixed lengths at 65536 strings (0.94 .. 1.13).
 * Applies to later calls; hrx_ctx_clone copies the options.  hrx_ctx_get_option: the value, -1 for an unknown option. */
enum { HRX_OPT_PMD_COMBINER_WAVE = 1, HRX_OPT_HOST_ROUTE = 2, HRX_OPT_HOST_THREADS = 3, HRX_OPT_HOST_PIPELINE = 4, HRX_OPT_PLACE_DRY_LAUNCH = 5, HRX_OPT_MATCH_FUSED_WIDE = 6 };
enum { HRX_HOST_ROUTE_AUTO = 0, HRX_HOST_ROUTE_DEVICE = 1, HRX_HOST_ROUTE_HOST = 2 };
/* What the context's last hrx_witness_batch_host call did. */
typedef struct hrx_host_route_report {
    int route;                    /* what the call did — 0: split between the device and the host cores, 1: device only, 2: host cores only */
    size_t device_strings, host_strings;
    double device_ms, host_ms;    /* wall time of each part (they run at the same time) */
    double call_ms;
    double device_alone_ns_per_row, host_alone_ns_per_row, split_ns_per_row;   /* the context's figures after the call (0: not measured yet): what HRX_HOST_ROUTE_AUTO picks its way by */
    double device_ns_per_row, host_ns_per_row;   /* ... of the two parts of a split call (both running at once): what the next split is made from */
    int host_threads;
    int device_pipelined;         /* the device part: 1 chunks pipelined over two streams, 0 one stream */
} hrx_host_route_report;
int hrx_ctx_host_route_report(const hrx_ctx *ctx, hrx_host_route_report *out, size_t out_bytes);   /* out_bytes = sizeof(hrx_host_route_report) of the caller's header: the struct may grow at its end */
int hrx_ctx_set_option(hrx_ctx *ctx, int option, long value);
long hrx_ctx_get_option(const hrx_ctx *ctx, int option);
/* thread-local text of the last failing call (any entry point) */
const char *hrx_last_error(void);

/* ------------------------------------------------------------------ */
/* The hot path: witness rows for a batch of strings                    */
/* ------------------------------------------------------------------ */
/*
 * One call = match_substrs' integer content (lib.rs:316-318, 339-348, 387-519, 593-764) for B strings.
 *   chars    B strings, string b at chars + b*stride, stride % 16 == 0, base 16-byte aligned
 *   lens     n_b (bytes of string b), n_b <= M
 *   M        max_chars_size (lib.rs:128): witness rows per string
 *   records  [B][M][D] u32: state_d[r] | substr_id_d[r] << 16 | start_enable_d[r] << 24 | end_enable_d[r] << 25
 *            (the states / substr_ids / start_enable / end_enable advice columns, lib.rs:419-519)
 *   masked   [B][M] u16:   masked_char[r] | masked_substr_id[r] << 8
 *            (AssignedRegexResult.masked_characters / .all_substr_ids, lib.rs:766-771)
 *   status   [B] u64: bits 0..7 code
 *            0 ok: bits 8..39 = accept mask (bit d: state at row n == accepted_state_val of def d, lib.rs:442-457)
 *            1 invalid transition (lib.rs:817): bits 8..15 def, 16..23 char, 24..39 state, 40..63 position;
 *              lowest def, then lowest position, like the reference's loop order
 *            2 two defs flag the same row (out of contract): bits 40..63 row
 *            3 n_b > M
 *            records/masked of a string whose code != 0 are unspecified.
 * Alignment (all the device entry points of this section; less is HRX_ERR_ARG, and nothing is written): chars, records, masked and every
 * record plane / row stripe 16 bytes, status 8 bytes, lens 4 bytes.  More is never needed: a caller may carve the buffers out of a pool
 * of its own at exactly these alignments.
 * All five pointers are DEVICE pointers on ctx's device; `stream` is a hipStream_t (NULL = the HIP null stream).
 * The call is asynchronous on that stream.
 */
int hrx_witness_batch_device(hrx_ctx *ctx, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B,
                             size_t M, uint32_t *records, uint16_t *masked, uint64_t *status, void *stream);
/* Same with pitched outputs: string b's rows start at records + b*rec_pitch*D and masked + b*msk_pitch (pitches in rows,
 * >= M, multiples of 8 when M is).  A pitch that is not a power of two keeps the chip-wide write front off a subset of the
 * HBM channels (NOTES_MEASUREMENTS.md §4); hrx_recommended_pitches gives values for a given M (and an input stride). */
int hrx_witness_batch_device_pitched(hrx_ctx *ctx, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B,
                                     size_t M, uint32_t *records, size_t rec_pitch, uint16_t *masked, size_t msk_pitch,
                                     uint64_t *status, void *stream);
void hrx_recommended_pitches(size_t M, size_t *rec_pitch, size_t *msk_pitch, size_t *chars_stride);
/* Output layouts of the device entry point below.
 *   HRX_LAYOUT_STRING_MAJOR   records [B][M][D], masked [B][M]                       (hrx_witness_batch_device)
 *   HRX_LAYOUT_POSITION_MAJOR records [ceil(M/4)][D][B][4], masked [ceil(M/8)][B][8] for B <= HRX_PM_BLOCK (65536):
 *       record of (string b, row r, def d) at ((r/4*D + d)*B + b)*4 + r%4;  masked of (b, r) at (r/8*B + b)*8 + r%8.
 *       Four rows of one string and def are 16 contiguous bytes and consecutive strings are adjacent, so with one GPU
 *       lane per string every store instruction writes one contiguous 1-KiB run of full lines, and the whole device
 *       writes into one compact slab at a time — the layout the HBM write path rewards (NOTES_MEASUREMENTS.md §4); rows >= M of
 *       the last quad/octet are unspecified.
 *       Larger batches are BLOCKED: strings [k*HRX_PM_BLOCK, (k+1)*HRX_PM_BLOCK) form block k, each block is a complete
 *       array of the above shape over its own nb = min(HRX_PM_BLOCK, B - k*HRX_PM_BLOCK) strings, blocks back to back:
 *       with k = b / HRX_PM_BLOCK, b' = b % HRX_PM_BLOCK,
 *         record at k*HRX_PM_BLOCK*ceil(M/4)*D*4 + ((r/4*D + d)*nb + b')*4 + r%4,
 *         masked at k*HRX_PM_BLOCK*ceil(M/8)*8   + (r/8*nb + b')*8 + r%8
 *       (the distance between a string's consecutive quads stays <= 1 MiB per def whatever B is: 14-28 % faster than one
 *       array over 262144 strings).  Buffer sizes: hrx_position_major_sizes.  The values equal the string-major ones.
 *   HRX_LAYOUT_INPUT_POSITION_MAJOR (or-ed with HRX_LAYOUT_POSITION_MAJOR): the input is chunked and blocked the same
 *       way, per block chars [stride/16][nb][16]: byte i of string b at k*HRX_PM_BLOCK*stride + ((i/16)*nb + b')*16 + i%16
 *       — what a caller that assembles the batch itself should write; `stride` is then only the per-string capacity
 *       (stride % 16 == 0, >= every n_b). */
#define HRX_PM_BLOCK 65536
enum { HRX_LAYOUT_STRING_MAJOR = 0, HRX_LAYOUT_POSITION_MAJOR = 1, HRX_LAYOUT_INPUT_POSITION_MAJOR = 2,
       HRX_LAYOUT_RECORD_PLANES = 4 /* hrx_describe_launch / hrx_ctx_describe_launch only, or-ed with HRX_LAYOUT_POSITION_MAJOR: the launch of hrx_witness_batch_device_planes */ };
int hrx_witness_batch_device_layout(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                                    size_t B, size_t M, uint32_t *records, uint16_t *masked, uint64_t *status, void *stream);
void hrx_position_major_sizes(size_t B, size_t M, size_t D, size_t *records_u32, size_t *masked_u16);
/* RECORD PLANES — HRX_LAYOUT_POSITION_MAJOR with every def's records in a buffer of its own: plane d holds the states / substr_ids / start_enable / end_enable
 * columns of regex_defs[d] (src/lib.rs:387-519 fills them per def), laid out like the position-major records of a one-def config — per block of HRX_PM_BLOCK
 * strings [ceil(M/4)][nb][4] u32, blocks back to back: record of (string b, row r) of def d at record_planes[d][k*HRX_PM_BLOCK*ceil(M/4)*4 + ((r/4)*nb + b')*4 + r%4];
 * masked, status, chars, lens and `layout` (HRX_LAYOUT_POSITION_MAJOR, optionally | HRX_LAYOUT_INPUT_POSITION_MAJOR) as in hrx_witness_batch_device_layout.
 * Why: a launch of D defs writes 4 D of its 4 D + 2 output bytes per row into the records; as ONE allocation they lie in one class of the MI355X's physical
 * address space and the launch runs at what one class absorbs, as separately placed planes (hrx_alloc_output_planes) its D + 1 write streams spread over the
 * classes: three defs x 32768 x 32768 rows 0.78-0.80 of the HBM peak against 0.70-0.72, two defs x 2^20 x 2048 rows 0.81 against 0.75-0.78 (DESIGN.md §6,
 * profiles/r06_probes/).
 * n_planes = the config's number of defs.  ONE def may also come in TWO ROW STRIPES (n_planes = 2): quad q = r/4 of a string lies in record_planes[q % 2] at slot q / 2,
 * each stripe per block [ceil(ceil(M/4)/2)][nb][4] — record of (b, r) at record_planes[(r/4) % 2][k*HRX_PM_BLOCK*ceil(ceil(M/4)/2)*4 + ((r/8)*nb + b')*4 + r%4] — so that
 * a one-def launch's record bytes spread over two classes beside the masked rows' third (sizes: hrx_position_major_stripe_sizes).
 * Configs that run as one launch (up to three defs, or four to eight defs of at most 32 byte classes each); the values equal the interleaved layout's. */
int hrx_witness_batch_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M,
                                    uint32_t *const *record_planes, size_t n_planes, uint16_t *masked, uint64_t *status, void *stream);
void hrx_position_major_plane_sizes(size_t B, size_t M, size_t *plane_u32, size_t *masked_u16);
void hrx_position_major_stripe_sizes(size_t B, size_t M, size_t n_stripes, size_t *stripe_u32, size_t *masked_u16);
/* The n_planes record buffers (the D planes; one def: 1, or 2 row stripes) and the masked rows of a batch of B strings x M rows, each allocated on ctx's device in a
 * neighbourhood of its own: a pool of n_planes + 4 record-sized and 5 masked-row-sized candidates, allocated one after the other (they walk down the device memory), is
 * measured pair by pair (two equal write streams, ~1 ms per pair on the device clock); pairings fall into two levels — both buffers in one class of the physical address
 * space, or not — and the buffers whose busiest class takes the fewest of the launch's output bytes per row (4 per plane — 2 per row stripe —, 2 for the masked rows; then
 * the fewest colliding pairings, the largest sum of pairings) are kept; a pool whose best set still collides (up to three buffers: at all; more: beyond one record buffer +
 * the masked rows) grows by three record candidates, at most twice; then the context's own launch of B strings x M rows runs over the (at most six) best sets by that
 * score, on a constant input, and the fastest is kept (the pairwise probe does not see everything: 2.5 ms against 2.9 per launch for sets it ranks alike); everything else
 * is freed before the call returns.  Record buffers below 1 GiB are carved out of up to
 * four 2-GiB STRIPE ARENAS per device and process chosen the same way once (a probe over buffers that fit the Infinity Cache would measure the cache); hrx_device_free gives
 * a sub-buffer's range back.  hrx_alloc_last_report: steps = pairings measured, ref_gbs = the slowest pairing seen, first_gbs = the slowest pairing of the first buffers
 * (what plain allocations would have been), best_gbs = the kept set's, chosen_step = the bytes per row of the kept set's busiest class, searched = 2: served from arenas
 * measured earlier.  The pool never takes more than 70 % of the free memory (hrx_ctx_set_placement narrows that and bounds the time).  Less than 128 MiB of records,
 * HRX_PLACE_OFF: plain allocations.  record_planes: n_planes pointers out; each buffer is released with hrx_device_free.  n_planes = 1: hrx_alloc_outputs_position_major.
 * Takes the context's lock; not inside a stream capture. */
int hrx_alloc_output_planes(hrx_ctx *ctx, size_t B, size_t M, size_t n_planes, uint32_t **record_planes, uint16_t **masked);
/* The same for a batch that already lies on the device: the launches that choose among the best sets run THE CALLER'S batch (chars, stride, lens, layout as
 * hrx_witness_batch_device_planes takes them: HRX_LAYOUT_POSITION_MAJOR, optionally | HRX_LAYOUT_INPUT_POSITION_MAJOR) instead of a constant stand-in, so where the input lies
 * and what the walk does with it are part of what is measured — the choice for a prover that keeps its input buffer and launches batch after batch into the outputs.  With it
 * one def's single buffer (n_planes = 1) also goes through the pool (on a stand-in input that lost against the pair walk: with one def the input is a seventh of the traffic,
 * profiles/r06_probes/cfg5_pool_dry.txt).  chars / lens must be complete on the device before the call (the launches run on the context's stream); the outputs they write are
 * the candidates', the batch itself is only read. */
int hrx_alloc_output_planes_for_batch(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M, size_t n_planes,
                                      uint32_t **record_planes, uint16_t **masked);
/* The allocator's measurement, for a caller that manages device memory itself (a prover with its own pool): two equal, time-aligned write streams over the first `bytes`
 * of device buffers a and b (both are OVERWRITTEN), *gbs = bytes written per time.  Pairings in one class of the physical address space measure 5.2-6.2 TB/s, in different
 * classes 6.5-7.3 (a level per box: compare pairings with each other, not with a constant).  Synchronous; takes the context's lock. */
int hrx_probe_write_pair(hrx_ctx *ctx, void *a, void *b, size_t bytes, double *gbs);
/* hrx_rows_of_string_position_major for record planes (or the two row stripes of one def) in HOST memory, each buffer copied from the device as it is: records [M][D], masked [M] of string b. */
int hrx_rows_of_string_planes(const uint32_t *const *record_planes, size_t n_planes, const uint16_t *masked_pm, size_t B, size_t M, size_t D, size_t b,
                              uint32_t *records, uint16_t *masked);
/* One circuit's view of a position-major batch, on the HOST: the rows of string b of a batch of B strings x M rows x D defs that lies in host memory in
 * HRX_LAYOUT_POSITION_MAJOR (e.g. copied from the device as it is) -> records [M][D] u32 and masked [M] u16, the string-major values the fill loops of
 * match_substrs index per string (src/lib.rs:387-519).  A string's consecutive quads are nb*16*D bytes apart, so this is M/4*D + M/8 gathers of 16 bytes:
 * ~10 us per 1024-row string on one core (bench.py: end_to_end_host.gather_us_per_string) against the ~(14 D + 21) gate calls per row that consume
 * them.  Either buffer pair may be NULL (records_pm with records, masked_pm with masked).  No context, no device, re-entrant. */
int hrx_rows_of_string_position_major(const uint32_t *records_pm, const uint16_t *masked_pm, size_t B, size_t M, size_t D, size_t b,
                                      uint32_t *records, uint16_t *masked);
/* Allocates the records and masked-row buffers of a position-major batch of B strings x M rows (sizes as
 * hrx_position_major_sizes) on ctx's device; each is released with hrx_device_free.  Optional — every entry point takes any
 * device pointer — and for records below 128 MiB (a launch that lives in the 256-MB Infinity Cache) just two hipMalloc calls.
 * From there on the call is PLACEMENT-AWARE: two concurrent write streams run ~15 % slower on an MI355X when they lie in the
 * same class of the physical address space (four classes, chosen by address bits >= 2^33) than when they do not, a launch
 * writes records and masked rows as two such streams, and buffers allocated one after the other come from one neighbourhood.
 * So the call walks down the device memory — block after block, each measured against the records with a two-stream write of
 * a few hundred microseconds that times itself on the device clock (robust under a profiler); the reference is the same probe
 * inside ONE block, a candidate that writes 10 % more bytes per time than that is taken, failing that the fastest measured, and everything else is freed
 * before the call returns; the walk never holds more than 70 % of the device memory that was free.
 *   records >= 1 GiB: the blocks are the masked-row candidates themselves, measured against the records buffer itself.
 *   records <  1 GiB: such buffers are carved out of two 2-GiB ARENAS per DEVICE and process (one for records, one for masked
 *     rows; a probe over buffers that fit the Infinity Cache would measure the cache, and the driver puts small blocks into any
 *     hole): the first such call of any context of the device finds the pair, later calls — of every context of that device:
 *     one context per worker thread shares one pair — are served from it until it is full (then a new pair is found);
 *     hrx_device_free returns a sub-buffer's range to its arena (it is handed out again: allocating and freeing per batch stays
 *     on one measured pair) and an arena is released with its last sub-buffer once the pair has been replaced or the device's
 *     last context is destroyed.  A process therefore holds up to 4 GiB per device for its small
 *     output buffers, however many contexts it keeps.
 * 262144 x 2048 B at D = 2 runs at 0.97-1.03 ms with such a pair against 1.12-1.19 ms in a fresh process with two plain
 * allocations (csrc/hrx_place.hip).  The call takes the context's lock, launches on the context's own stream
 * and waits for it: not inside a stream capture.  Per context: hrx_ctx_set_placement (off / on, memory and time budget of a walk).
 * Environment, read by hrx_ctx_create (the defaults of a new context): HRX_PLACE=0 (plain allocations), HRX_PLACE_MAX_STEPS,
 * HRX_PLACE_TRACE=1.  The reference has no counterpart: its witness lives in host Vecs. */
int hrx_alloc_outputs_position_major(hrx_ctx *ctx, size_t B, size_t M, uint32_t **records, uint16_t **masked);
/* The same for any pair of output buffers given in bytes (string-major outputs: B * rec_pitch * D * 4 and B * msk_pitch * 2). */
int hrx_alloc_output_pair(hrx_ctx *ctx, size_t records_bytes, size_t masked_bytes, void **records, void **masked);
/* What the context's last hrx_alloc_output_pair / hrx_alloc_outputs_position_major call did. */
typedef struct hrx_place_report {
    int searched;                /* 0: two plain allocations (small buffers, HRX_PLACE=0, or no memory to walk with); 1: this call walked;
                                    2: served from the arena pair an earlier call measured (the numbers below are that walk's) */
    int steps;                   /* candidates measured */
    int accepted;                /* 1: the kept candidate is >= 10 % above both the same-neighbourhood reference and the MEDIAN candidate of the walk (at
                                    least four candidates; eight in a context's first direct walk) and within 4 % of the best pairing earlier walks of the same kind measured — or a walk that ran
                                    into a bound with a candidate >= 10 % above the reference in hand; 0: simply the fastest measured (csrc/hrx_place_rule.hpp) */
    int chosen_step;
    double ref_us;               /* the reference: both probe streams inside one neighbourhood (device clock) */
    double first_us, best_us;    /* the first candidate (what two plain allocations would have been) and the kept one */
    double ref_gbs, first_gbs, best_gbs;   /* the same three as bytes written per time (GB/s): what acceptance compares — the reference pass
                                    writes fewer bytes than a candidate pass */
    size_t probe_bytes;          /* bytes one probe pass writes */
    size_t peak_candidate_bytes; /* most memory the walk held at once: rejected candidates stay allocated, as the spacers that push the
                                    next candidate further, until the walk ends */
    double search_ms;            /* host time of the whole call */
    int capped;                  /* which bound ended the walk, if one did (0: the acceptance rule itself): HRX_PLACE_CAPPED_* or-ed */
} hrx_place_report;
enum {
    HRX_PLACE_CAPPED_STEPS = 1,  /* the candidate count (48; 2-GiB arena candidates 96; HRX_PLACE_MAX_STEPS) */
    HRX_PLACE_CAPPED_BYTES = 2,  /* the memory budget: 70 % of the free memory, hrx_ctx_set_placement's max_bytes, or — arena walks past their 24th
                                    candidate — less than 30 % of the device left free */
    HRX_PLACE_CAPPED_TIME = 4,   /* hrx_ctx_set_placement's max_ms, or the rule's own hard bound (2 s; arena walks 8 s) */
    HRX_PLACE_CAPPED_ALLOC = 8   /* a candidate could not be allocated */
};
int hrx_alloc_last_report(const hrx_ctx *ctx, hrx_place_report *out);
/* The same into a buffer of out_bytes: min(out_bytes, sizeof(hrx_place_report)) bytes are written.  hrx_place_report only ever grows at its end (`capped` came in round 5), so a
 * consumer built against an earlier header passes the size of ITS struct and gets the fields it knows (hrx_alloc_last_report writes the whole current struct). */
int hrx_alloc_last_report_sized(const hrx_ctx *ctx, void *out, size_t out_bytes);
/* Placement per context (a prover that links the library decides per context, not through the environment):
 *   mode       HRX_PLACE_OFF: hrx_alloc_output_pair / hrx_alloc_outputs_position_major are two plain allocations, nothing is measured, no arena is held
 *              on this context's behalf; HRX_PLACE_WALK (the default unless HRX_PLACE=0 was set when the context was created): as described above.
 *   max_bytes  the most device memory one walk may hold at a time in candidates (0: 70 % of what is free when the walk begins; never more than that)
 *   max_ms     wall-clock bound of one walk in milliseconds (0: the rule's own bounds); the walk keeps the fastest candidate measured until then
 * A walk that ends on a bound says so in hrx_place_report.capped.  Applies to later calls; buffers already handed out are not touched. */
enum { HRX_PLACE_OFF = 0, HRX_PLACE_WALK = 1 };
int hrx_ctx_set_placement(hrx_ctx *ctx, int mode, size_t max_bytes, double max_ms);
/* Roofline diagnostic: the memory traffic of ONE position-major witness launch of B strings x M rows of this context's
 * config (HRX_LAYOUT_POSITION_MAJOR | HRX_LAYOUT_INPUT_POSITION_MAJOR) and nothing else — the input read in 16-byte chunks
 * per lane, every record plane and the masked rows written at the launch's own addresses with the launch's store policy, by
 * four reader and four writer waves per CU — no DFA work.  OVERWRITES records and masked with junk.  What it takes is this
 * box's ceiling for the launch's byte mix on these very buffers (bench.py: roofline.mix_ceiling).  Asynchronous on `stream`. */
int hrx_traffic_pass_device(hrx_ctx *ctx, const uint8_t *chars, size_t stride, size_t B, size_t M, uint32_t *records,
                            uint16_t *masked, void *stream);
/* The same diagnostic for either layout: HRX_LAYOUT_POSITION_MAJOR | HRX_LAYOUT_INPUT_POSITION_MAJOR is the call above (pitches ignored);
 * HRX_LAYOUT_STRING_MAJOR moves the bytes of a string-major launch (M % 8 == 0) the way the walker/storer kernel does — a store instruction writes the 128-byte
 * lines of eight strings, 2 D lines of records and one of masked rows per string and 64 rows, the input read one string per lane — rec_pitch / msk_pitch in rows
 * (0 = M).  What the string-major lines of a sweep are measured against (the reference's fill loops index one string: src/lib.rs:387-519). */
int hrx_traffic_pass_device_layout(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, size_t B, size_t M, uint32_t *records, size_t rec_pitch,
                                   uint16_t *masked, size_t msk_pitch, void *stream);
/* ... over record planes (hrx_witness_batch_device_planes): the same traffic with plane d written at record_planes[d]. */
int hrx_traffic_pass_device_planes(hrx_ctx *ctx, const uint8_t *chars, size_t stride, size_t B, size_t M, uint32_t *const *record_planes, size_t n_planes,
                                   uint16_t *masked, void *stream);
/* From the reference's input shape to the coalesced one, on the device: `chars` = B strings of `stride` bytes each, back to back — one contiguous
 * &[u8] per string is what RegexVerifyConfig::match_substrs is handed (src/lib.rs:311-315) — -> `chars_pm` (B * stride bytes, another buffer) in
 * HRX_LAYOUT_INPUT_POSITION_MAJOR.  Pure streaming (2 * stride bytes of traffic per string; measured beside the bench line: bench.py
 * roofline.from_string_major_input).  Asynchronous on `stream`; no context state is touched. */
int hrx_chars_to_position_major_device(hrx_ctx *ctx, const uint8_t *chars, size_t stride, size_t B, uint8_t *chars_pm, void *stream);
/* Releases a buffer of hrx_alloc_output_pair / hrx_alloc_outputs_position_major / hrx_alloc_output_planes (NULL: nothing).  As with hipFree, the memory is not
 * handed out again before the buffer's device has finished everything in flight, so a buffer may be freed while the launch that writes it is still running.  A buffer of
 * its own: hipFree (which waits).  A sub-buffer of a shared arena: the call returns at once — from any thread, also while another thread captures a stream — and the range
 * is parked; a later allocation whose request does not fit otherwise waits for the device once and takes the parked ranges back. */
int hrx_device_free(void *ptr);
/* Which kernel and launch geometry the planner picks for a batch of B strings x M rows in `layout` on a gfx950 device
 * with `num_cus` compute units (MI355X: 256), as text: "hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256
 * waves=12 ring=4 lds=..." — the kernel name a profiler will show, every template argument spelled out (bench.py's roofline.kernel).  Host-only: nothing is
 * launched and no device is touched.  Returns HRX_OK, HRX_ERR_BOUNDS if nothing fits. */
int hrx_describe_launch(const hrx_defs *defs, int layout, size_t B, size_t M, int num_cus, char *out, size_t cap);
/* The same for a context: its own device's CU count (256 on a host-only context), the kernel-selection flags it was created with and its hrx_ctx_set_option choices. */
int hrx_ctx_describe_launch(const hrx_ctx *ctx, int layout, size_t B, size_t M, char *out, size_t cap);
/* Same with HOST buffers (any alignment/stride >= max len): staged through ctx-owned device buffers, or — below the
 * context's host threshold, and always on a host-only context — walked on the host; synchronous.  This is what an unmodified caller of
 * match_substrs' seam gets (host Vecs in, host Vecs out, src/lib.rs:311-318).  Batches of more than ~100 MiB of rows go one of two ways: pipelined chunk by chunk
 * (a staging thread copies chunk c in and launches its walk while the calling thread copies chunk c - 1's rows out on a second stream), or in, walk, out on one stream —
 * the context times both over its first calls and keeps the faster one for this process on this box (the pipeline's copies out run at half rate on some hosts), looking again
 * every 64 calls; the call lasts about as long as the copy out — (4 D + 2) bytes per row over the PCIe link in one direction (bench.py: end_to_end_host).
 * Environment: HRX_HOST_PIPELINE=1 / 0 forces a way, HRX_HOST_TRACE=1 prints a line per call on stderr, HRX_HOST_CHUNK_MIB the pipeline's chunk size. */
int hrx_witness_batch_host(hrx_ctx *ctx, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B,
                           size_t M, uint32_t *records, uint16_t *masked, uint64_t *status);

/* ------------------------------------------------------------------ */
/* MATCH: status + revealed spans of B strings, no witness rows         */
/* ------------------------------------------------------------------ */
/*
 * For callers that need only whether a string matches and what it reveals (the circuit's public instances,
 * lib.rs:1046-1058): no records, no masked rows, nothing of the witness's (4 D + 2) bytes per row leaves the device.
 *   status       [B] u64, bit for bit what hrx_witness_batch_device writes for the same batch
 *   span_counts  [B] u32: number of revealed RUNS of string b (may exceed max_spans); 0 when the status code != 0
 *   spans        [B][max_spans] u64: the first min(count, max_spans) runs in increasing start order; entries beyond are unspecified
 *                run = maximal range of rows r < n_b on which masked_substr_id[r] (lib.rs:752-761) is one non-zero value
 *                bits 0..27 start row, 28..55 length, 56..63 masked_substr_id
 *   max_spans    <= 2^16; 0: status only (span_counts may then be NULL, spans must be NULL)
 *   layout       HRX_LAYOUT_STRING_MAJOR (chars [B][stride]) or HRX_LAYOUT_INPUT_POSITION_MAJOR (blocked as for the witness)
 * Argument rules as for the witness entry points (alignment, M <= 2^24, stride % 16 == 0); span_counts and spans 8-byte aligned.
 * The device entry is asynchronous on `stream`.  Def sets the fused match kernel walks (hrx_ctx_describe_match names it) need no
 * scratch, and the call is then legal inside a stream capture; every other def set goes "via rows": the witness launch into
 * context-owned scratch (at most 1 GiB, allocated at first use: inside a capture before that, HRX_ERR_STATE; HRX_ERR_BOUNDS if one string's
 * witness rows alone would not fit) and a scan of its masked rows.  With HRX_OPT_MATCH_FUSED_WIDE = 1 the def sets of four to eight defs that the option
 * covers have a fused kernel too: no scratch, and the call can be captured on a fresh context.
 * hrx_match_batch_host: HOST buffers, synchronous; on a host-only context the native host walk, otherwise staged through the device. */
int hrx_match_batch_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M,
                           uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, void *stream);
int hrx_match_batch_host(hrx_ctx *ctx, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M,
                         uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans);
/* Which kernel(s) hrx_match_batch_device runs for a shape, as text (as hrx_describe_launch; host-only, nothing launched). */
int hrx_describe_match(const hrx_defs *defs, int layout, size_t B, size_t M, int num_cus, char *out, size_t cap);
int hrx_ctx_describe_match(const hrx_ctx *ctx, int layout, size_t B, size_t M, char *out, size_t cap);

/* ------------------------------------------------------------------ */
/* RAGGED input: strings back to back in one byte buffer + B + 1 offsets */
/* ------------------------------------------------------------------ */
/*
 * string b = values[offsets[b] .. offsets[b+1]), n_b = offsets[b+1] - offsets[b]; offsets has B + 1 entries (an Arrow large-binary column:
 * no string is padded).  offsets[0] need not be 0 and offsets may point at any byte: offsets + begin (with the same values) is a valid
 * slice of a larger column, which is how a caller shards one.  A string whose offsets decrease (offsets[b+1] < offsets[b]) or with
 * n_b > M gets kStatusBadLength (status code 3, the code the padded entry points give lens[b] > M) and count 0; none of its bytes are read.
 *
 * hrx_match_batch_device_ragged / hrx_match_batch_host_ragged: status, span_counts and spans are bit for bit what hrx_match_batch_device /
 *   hrx_match_batch_host return for the same strings padded into [B][stride] with lens[b] = n_b.
 *   Device entry: values 16-byte aligned, offsets 8-byte aligned.  The call reads whole aligned 16-byte chunks, so values must be readable
 *   up to round_up(offsets[B], 16) (in general: up to the aligned chunk end of every string's last byte), and it never reads a chunk that
 *   holds no byte of some string of the batch.  Every other argument rule, the asynchronous behaviour and the stream-capture rules are those
 *   of hrx_match_batch_device: where the fused kernel runs (hrx_ctx_describe_match with HRX_LAYOUT_INPUT_RAGGED names it) no scratch is
 *   needed and the launch can be captured (HRX_OPT_MATCH_FUSED_WIDE = 1: that holds for the four- to eight-def sets the option covers as well); "via rows" uses the
 *   context scratch with the same first-use and capture rules.
 *   Host entry: host buffers (no alignment rule for values), synchronous.  On a host-only context the native host walk; on a device
 *   context chunks of whole strings whose bytes span about 64 MiB go through the device, each one contiguous byte range plus its offsets
 *   in, status / counts / spans out.
 * hrx_ragged_to_position_major_device: the batch as HRX_LAYOUT_INPUT_POSITION_MAJOR input blocked by HRX_PM_BLOCK, per-string capacity
 *   `stride` (stride % 16 == 0): chars_pm [B * stride] bytes (16-byte aligned), the bytes past n_b zero, lens[b] = n_b.  A string longer than
 *   stride or with decreasing offsets gets lens[b] = UINT32_MAX (every consumer then reports kStatusBadLength for it).  The output feeds
 *   hrx_witness_batch_device_layout, hrx_witness_batch_device_planes, hrx_fr_columns_device* and hrx_match_batch_device unchanged: the
 *   ragged counterpart of hrx_chars_to_position_major_device.  Asynchronous on `stream`, no scratch, capturable. */
enum { HRX_LAYOUT_INPUT_RAGGED = 8 /* hrx_describe_match / hrx_ctx_describe_match only: the launch of hrx_match_batch_device_ragged */ };
int hrx_match_batch_device_ragged(hrx_ctx *ctx, const uint8_t *values, const uint64_t *offsets, size_t B, size_t M,
                                  uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, void *stream);
int hrx_match_batch_host_ragged(hrx_ctx *ctx, const uint8_t *values, const uint64_t *offsets, size_t B, size_t M,
                                uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans);
int hrx_ragged_to_position_major_device(hrx_ctx *ctx, const uint8_t *values, const uint64_t *offsets, size_t B,
                                        size_t stride, uint8_t *chars_pm, uint32_t *lens, void *stream);

/* ------------------------------------------------------------------ */
/* EXTRACT: the revealed bytes of a matched batch as an Arrow list<large_binary> column */
/* ------------------------------------------------------------------ */
/*
 * A match call reports WHERE a string reveals something (row numbers); this turns its outputs into WHAT is revealed, without the input leaving
 * the memory it is in.  For B strings with R revealed runs in total:
 *   run_offsets   [B + 1] u64         string b's runs are run indices [run_offsets[b], run_offsets[b + 1]); run_offsets[B] = R
 *   runs          [runs_cap] u64      run j's span word as the match call packed it (start row, length, masked_substr_id), in string order, then start order
 *   byte_offsets  [runs_cap + 1] u64  run j's bytes are values[byte_offsets[j] .. byte_offsets[j + 1])
 *   values        [values_cap] u8     the revealed bytes back to back, no padding
 *   totals        [4] u64             [0] R needed, [1] bytes needed, [2] contributing strings whose span_counts[b] > max_spans (the match call
 *                                     truncated them), [3] 0
 * String b contributes k_b = min(span_counts[b], max_spans) runs where its status code is 0 and ((status[b] >> 8) & require_accept) == require_accept,
 * else none: require_accept = 0 takes every string with status code 0, the mask of all defs only strings the circuit would accept.
 * CAPACITY: run_offsets and totals are always complete.  Run j is stored (runs[j], byte_offsets[j], byte_offsets[j + 1], its bytes) iff j < runs_cap and
 * byte_offsets[j + 1] <= values_cap; both conditions are monotone, so the stored runs are a prefix [0, J), byte_offsets[0 .. J] is written (byte_offsets[0] = 0)
 * and nothing at or beyond runs[runs_cap], byte_offsets[runs_cap + 1] or values[values_cap].  The caller compares totals with its caps; caps that always
 * suffice: runs_cap = B * max_spans, values_cap = the input's byte count (B * stride, or offsets[B] - offsets[0]).
 * DEFENSIVE: the span words are caller memory.  A run whose range leaves its string — [0, stride) of a padded slot, [0, n_b) of a ragged string — is clipped to
 * it (byte_offsets shows the clipped length; runs[j] stays the word as given); a ragged string with decreasing offsets contributes nothing.  No byte is read
 * that a match call on the same input may not read.
 *   layout        HRX_LAYOUT_STRING_MAJOR (src [B][stride]), HRX_LAYOUT_INPUT_POSITION_MAJOR (blocked by HRX_PM_BLOCK, stride % 16 == 0; device form only) or
 *                 HRX_LAYOUT_INPUT_RAGGED (src = values, offsets [B + 1], stride ignored); otherwise offsets is ignored
 *   status, span_counts, spans   the outputs of a match call on the same input with the same max_spans, 1 <= max_spans <= 2^16
 * All u64 arrays 8-byte aligned, span_counts 4-byte; stride <= 2^28.
 * Device form: device pointers, asynchronous on `stream`: four kernel launches and nothing else — no allocation, no context scratch, no synchronisation — so it is
 * legal inside a stream capture whatever def set the context holds, and deterministic.  Its temporaries live in `workspace` (8-byte aligned device memory of
 * at least hrx_extract_workspace_bytes(B) bytes; too small: HRX_ERR_ARG).  HRX_ERR_HIP on a host-only context.
 * Host form: host pointers, no context, re-entrant; threads <= 0: as many as the host has.  It serves host-only and device contexts alike, since the input
 * bytes are in host memory already: the host route is a host match call followed by this, and no values travel back over the link. */
typedef struct hrx_extract_out {
    uint64_t *run_offsets; uint64_t *runs; uint64_t *byte_offsets; uint8_t *values;
    uint64_t *totals; size_t runs_cap; size_t values_cap;
} hrx_extract_out;
size_t hrx_extract_workspace_bytes(size_t B);
int hrx_extract_spans_device(hrx_ctx *ctx, int layout, const uint8_t *src, size_t stride, const uint64_t *offsets, size_t B,
                             const uint64_t *status, const uint32_t *span_counts, const uint64_t *spans, size_t max_spans,
                             uint32_t require_accept, const hrx_extract_out *out, void *workspace, size_t workspace_bytes, void *stream);
int hrx_extract_spans_host(int layout, const uint8_t *src, size_t stride, const uint64_t *offsets, size_t B,
                           const uint64_t *status, const uint32_t *span_counts, const uint64_t *spans, size_t max_spans,
                           uint32_t require_accept, const hrx_extract_out *out, int threads);

/* ------------------------------------------------------------------ */
/* ROUTE: a screened batch sorted into circuit-size buckets and staged as witness input */
/* ------------------------------------------------------------------ */
/*
 * The step between "screen" (a match call) and "prove" (a witness call per circuit size): M is a per-call argument of every witness entry point and the
 * witness writes (4 D + 2) * M bytes per string whatever n_b is, so a caller with proving keys for several sizes wants each string witnessed at the smallest
 * size that takes it, and the strings the circuit would not accept not witnessed at all — without status, offsets or bytes leaving the device.
 *
 * hrx_route_device / hrx_route_host: a stable partition of strings 0..B by (kept?, length bucket).
 *   lens / offsets  exactly one is non-NULL (else HRX_ERR_ARG): lens [B] u32 as the padded entry points take it, n_b = lens[b]; or offsets [B + 1] u64 as the
 *                   ragged ones take it, n_b = offsets[b+1] - offsets[b] (a string whose offsets decrease has no valid length)
 *   status          [B] u64 of a match call on the same strings, or NULL: no screening.  String b passes the screen iff its status code is 0 and
 *                   ((status[b] >> 8) & require_accept) == require_accept — the rule of hrx_extract_spans_*
 *   bounds          [n_buckets] u32, a HOST array in both forms (read at call time): the circuit sizes, 1 <= n_buckets <= HRX_MAX_BUCKETS, strictly
 *                   increasing, bounds[n_buckets - 1] <= 2^24; B < 2^32.  Anything else: HRX_ERR_ARG
 * String b is KEPT iff it passes the screen, its length is valid and n_b <= bounds[n_buckets - 1]; its bucket is the least j with n_b <= bounds[j]
 * (n_b == bounds[j] belongs to bucket j: the witness accepts n == M).
 *   order           [B] u32: a permutation of 0..B
 *   bucket_offsets  [n_buckets + 2] u64: bucket j is order[bucket_offsets[j] .. bucket_offsets[j+1]); range j == n_buckets holds the strings that were NOT
 *                   kept, so that a front-end can report its rejects.  bucket_offsets[0] = 0, bucket_offsets[n_buckets + 1] = B.
 * Every range is in increasing b: the partition is stable, and the result is deterministic.
 * status, offsets and bucket_offsets 8-byte aligned, lens and order 4-byte.
 * Device form: device pointers (bounds excepted), asynchronous on `stream`: three kernel launches and nothing else — no allocation, no context scratch, no
 * synchronisation, no atomics — so it is legal inside a stream capture whatever def set the context holds.  Its temporaries live in `workspace` (8-byte
 * aligned device memory of at least hrx_route_workspace_bytes(B) bytes; too small: HRX_ERR_ARG).  HRX_ERR_HIP on a host-only context.  B == 0 writes
 * bucket_offsets (all zero) and reads nothing.
 * Host form: host pointers, no context, re-entrant, sequential, nothing allocated.
 *
 * hrx_gather_to_position_major_device: the strings sel[0 .. n_sel) of a batch of B as HRX_LAYOUT_INPUT_POSITION_MAJOR input blocked by HRX_PM_BLOCK over the
 * OUTPUT index k, per-string capacity `stride` (stride % 16 == 0, >= 16): chars_pm [n_sel * stride] bytes (16-byte aligned), slot k holds source string
 * sel[k], the bytes past its n zero, lens_out[k] = n.  Typically sel = order + bucket_offsets[j] and stride = round_up(bounds[j], 16), after the caller has
 * read bucket_offsets back ((n_buckets + 2) * 8 bytes).  The output feeds hrx_witness_batch_device_layout, hrx_witness_batch_device_planes,
 * hrx_fr_columns_device* and hrx_match_batch_device unchanged, called with M = bounds[j].
 *   layout  HRX_LAYOUT_STRING_MAJOR: src [B][src_stride] (16-byte aligned, src_stride % 16 == 0), lens [B]; offsets ignored
 *           HRX_LAYOUT_INPUT_RAGGED: src = values, offsets [B + 1]; alignment and readable range as for hrx_ragged_to_position_major_device; src_stride, lens ignored
 *   sel     [n_sel] u32 device array of string indices, in any order, repeats allowed
 * DEFENSIVE: sel is caller memory.  Slot k is all zero with lens_out[k] = UINT32_MAX, and none of that string's bytes is read, when sel[k] >= B, a ragged
 * string's offsets decrease, n > stride, or (string-major) lens[sel[k]] > src_stride; every consumer then reports kStatusBadLength for that slot.
 * Asynchronous on `stream`, one launch, no scratch, capturable.  HRX_ERR_HIP on a host-only context.  (hrx_ragged_to_position_major_device is the same kernel
 * without sel; hrx_chars_to_position_major_device stays the faster route for a dense, unselected string-major batch.) */
#define HRX_MAX_BUCKETS 8
size_t hrx_route_workspace_bytes(size_t B);
int hrx_route_device(hrx_ctx *ctx, const uint64_t *status, uint32_t require_accept,
                     const uint32_t *lens, const uint64_t *offsets, size_t B,
                     const uint32_t *bounds, size_t n_buckets,
                     uint32_t *order, uint64_t *bucket_offsets,
                     void *workspace, size_t workspace_bytes, void *stream);
int hrx_route_host(const uint64_t *status, uint32_t require_accept,
                   const uint32_t *lens, const uint64_t *offsets, size_t B,
                   const uint32_t *bounds, size_t n_buckets,
                   uint32_t *order, uint64_t *bucket_offsets);
int hrx_gather_to_position_major_device(hrx_ctx *ctx, int layout, const uint8_t *src, size_t src_stride,
                                        const uint32_t *lens, const uint64_t *offsets, size_t B,
                                        const uint32_t *sel, size_t n_sel,
                                        size_t stride, uint8_t *chars_pm, uint32_t *lens_out, void *stream);

/* ------------------------------------------------------------------ */
/* SELECTED: match a selection of a batch through an index array, in its order */
/* ------------------------------------------------------------------ */
/*
 * hrx_match_selected_device / hrx_match_selected_host: the match of strings sel[0 .. n_sel) of a batch of B, and of no other.  What a second, more
 * expensive screen runs over the survivors of a first one (sel = the kept ranges of hrx_route's order), or what walks a batch in length order
 * (sel = the order of hrx_route with status = NULL), without a copy of the strings.
 *   SOURCE     layout, src, src_stride, lens, offsets and B describe the source batch exactly as hrx_gather_to_position_major_device takes it:
 *              HRX_LAYOUT_STRING_MAJOR (src [B][src_stride], lens [B]; offsets ignored) or HRX_LAYOUT_INPUT_RAGGED (src = values, offsets [B + 1];
 *              src_stride and lens ignored).  Alignment and readable range are those of hrx_match_batch_device / hrx_match_batch_device_ragged (device
 *              entry: src 16-byte aligned, src_stride % 16 == 0 and >= 16; the host entry has no alignment rule for src).  Position-major input is
 *              refused with HRX_ERR_ARG: it is dense by construction, and hrx_match_batch_device serves it.
 *   SELECTION  sel [n_sel] u32, 4-byte aligned: a device array for the device entry, a host array for the host entry; what hrx_route_device writes as
 *              `order`.  Entries are distinct: the result for a repeated index is unspecified.  An entry >= B is skipped: nothing is read for it and
 *              nothing is written.  n_sel == 0 launches nothing; sel == NULL with n_sel > 0 is HRX_ERR_ARG.
 *   OUTPUTS    are indexed by STRING, not by slot: status [B], span_counts [B], spans [B][max_spans], the sizes and rules of the unselected call.  For
 *              every b in sel the entries of b are bit for bit what the unselected entry of the same layout writes, kStatusBadLength with count 0
 *              included: decreasing offsets, n_b > M, or lens[b] > src_stride (none of that string's bytes are read).  Entries of strings not in sel
 *              are not touched: a caller pre-fills them or reads only the selected ones.  hrx_extract_spans_* and hrx_route_* therefore run behind
 *              this call unchanged (pre-fill status with kStatusBadLength = 3 and the counts with 0 for "not matched").
 *   ORDER      the strings are walked in sel order: persistent lane g of G takes sel[g], sel[g + G], ...  Order affects time only.
 * The device entry is asynchronous on `stream`; stream-capture and scratch rules are those of hrx_match_batch_device_ragged: def sets with a fused
 * kernel need no scratch and the launch can be captured; "via rows" def sets use the context scratch with the same first-use rule (inside a capture
 * before that: HRX_ERR_STATE); HRX_OPT_MATCH_FUSED_WIDE = 1 gives the four- to eight-def sets it covers a fused kernel here too.  No atomics: the call is deterministic.  HRX_ERR_HIP on a host-only context (after the argument rules).
 * Host entry: host buffers, synchronous.  On a host-only context the native host walk over the selection; on a device context chunks of the selection
 * whose strings' bytes sum to about 64 MiB are packed back to back, matched on the device and copied out to index sel[k]: only the selected strings'
 * bytes cross the link.
 * hrx_describe_match / hrx_ctx_describe_match accept HRX_LAYOUT_INPUT_SELECTED or-ed with one of the two source layouts, with B standing for n_sel, and
 * name this launch; the flag has a meaning only there. */
enum { HRX_LAYOUT_INPUT_SELECTED = 16 };
int hrx_match_selected_device(hrx_ctx *ctx, int layout, const uint8_t *src, size_t src_stride, const uint32_t *lens,
                              const uint64_t *offsets, size_t B, const uint32_t *sel, size_t n_sel, size_t M,
                              uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, void *stream);
int hrx_match_selected_host(hrx_ctx *ctx, int layout, const uint8_t *src, size_t src_stride, const uint32_t *lens,
                            const uint64_t *offsets, size_t B, const uint32_t *sel, size_t n_sel, size_t M,
                            uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans);

/* ------------------------------------------------------------------ */
/* SURVEY §8 f4 — compact witness -> field cells (the step after the path)        */
/* ------------------------------------------------------------------ */
/* Expands the compact rows of strings [b_begin, b_begin + b_count) of a finished batch into what
 * `Value::known(F::from(v))` holds for every advice cell the reference assigns (src/lib.rs:339-418, 473-519) and for the
 * two result columns of AssignedRegexResult (lib.rs:752-771), with F = halo2curves bn256::Fr, the field the reference's
 * circuits use (lib.rs:896): 4 little-endian u64 limbs per cell in Montgomery form (v * 2^256 mod r — the in-memory
 * representation of Fr, so that a device-side prover or an `assign_advice` loop can take the cells as they are);
 * HRX_FR_CANONICAL in `flags`: the plain integer instead.
 * cells: device buffer [n_cols][b_count][M][4] u64, n_cols = hrx_fr_num_columns(D) = 4 + 4 D, in column order
 *   0 char_enable, 1 characters, 2+4d states[d], 3+4d substr_ids[d], 4+4d start_enable[d], 5+4d end_enable[d],
 *   2+4D masked_characters, 3+4D all_substr_ids.
 * `layout`, chars/stride/lens, records/masked (and rec_pitch/msk_pitch, string-major only; 0 = M) are those of the
 * hrx_witness_batch_device* call that produced the rows.  Any b_count (served 32768 strings per launch).  Asynchronous on `stream`. */
enum { HRX_FR_CANONICAL = 1 };
size_t hrx_fr_num_columns(size_t D);
int hrx_fr_columns_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                          const uint32_t *records, size_t rec_pitch, const uint16_t *masked, size_t msk_pitch, size_t B,
                          size_t M, size_t b_begin, size_t b_count, uint64_t *cells, int flags, void *stream);
/* The same out of RECORD PLANES (hrx_witness_batch_device_planes: the D planes, or the two row stripes of one def); `layout` position-major, optionally | HRX_LAYOUT_INPUT_POSITION_MAJOR. */
int hrx_fr_columns_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *const *record_planes, size_t n_planes,
                                 const uint16_t *masked, size_t B, size_t M, size_t b_begin, size_t b_count, uint64_t *cells, int flags, void *stream);
/* F::from(v) on the host (same arithmetic as the kernel): limbs[4]. */
void hrx_fr_from_u64(uint64_t v, int flags, uint64_t *limbs);

/* ------------------------------------------------------------------ */
/* VERIFY — do these witness rows satisfy the circuit?  (what MockProver::verify() says of a witness, src/lib.rs:1086 ...) */
/* ------------------------------------------------------------------ */
/* Every gate and lookup of RegexVerifyConfig::configure (src/lib.rs:126-305) and the accept chain (lib.rs:427-457), evaluated over plain integers on the
 * compact rows of a finished batch — rows kept between runs, produced on another device or under a context option, read back after a fault — plus three
 * checks beyond what verify() sees, which pin the rest of the assignment.  One u64 verdict per string, 0 = every check holds:
 *   bits 0..8   the checks that fail
 *     HRX_VERIFY_FIRST_STATE   gate "The state must start from the first state value"   lib.rs:173-191
 *     HRX_VERIFY_ENABLE        gate "The transition of enable flags"                    lib.rs:193-205  (enable is [r < n_b]: cannot fail; kept gate for gate)
 *     HRX_VERIFY_TRANSITION    lookup "characters and their state"                      lib.rs:207-233
 *     HRX_VERIFY_START_LOOKUP  lookup "start_state of substring"                        lib.rs:235-259
 *     HRX_VERIFY_END_LOOKUP    lookup "end_state of substring"                          lib.rs:261-284
 *     HRX_VERIFY_ACCEPT        accept chain: the state where enable drops is the accepted one   lib.rs:427-457
 *     (these six are HRX_VERIFY_CIRCUIT_BITS: what verify() itself sees; with n_b == M the transition and end lookups of row M - 1 read a cell
 *      match_substrs never assigns and are left out)
 *     HRX_VERIFY_FLAGS         start_enable / end_enable are exactly derive_is_start_end's (lib.rs:847-888) gated by enable (lib.rs:482-519)
 *     HRX_VERIFY_PADDING       rows from n_b on hold no tag and no flag, rows after n_b the dummy state (lib.rs:387-418); no flag bit above the two
 *     HRX_VERIFY_MASK          masked rows = the reveal gates (lib.rs:593-764) evaluated on the records' own sums; not reported for a string in which
 *                              two defs flag one row (out of contract)
 *   bits 32..56 the lowest row at which any reported check fails (0 when none does).  A check belongs to the row r whose record, masked cell or
 *               Rotation::next pair (r, r + 1) it reads; the accept chain to the row where enable drops; the first-state gate to row 0
 *   everything else 0.  n_b > M: all ones (the string has no rows).
 * The fixed tables are the rows RegexTableConfig::load assigns (hrx_table_transition_rows / hrx_table_endpoint_rows), never a walk's table: the
 * checker shares nothing with the kernels whose rows it judges.  They are built — and for the device forms uploaded — at the context's FIRST verify
 * call: inside a stream capture before that the device forms return HRX_ERR_STATE; afterwards a call is one kernel launch, asynchronous on `stream`,
 * and capturable.
 * `layout`, chars / stride / lens, records / masked (rec_pitch / msk_pitch string-major only, in rows; 0 = M) and the record planes are those of the
 * hrx_witness_batch_device* call that wrote the rows, at that section's alignments (and stride % 16 == 0); M <= 2^24; planes only with a
 * position-major layout, one per def (at most eight) or the two row stripes of one def.  verdict: [B] u64, 8-byte aligned.  A refused call writes
 * nothing.  The launch reads 1 + 4 D + 2 bytes per row once and writes 8 bytes per string. */
enum { HRX_VERIFY_FIRST_STATE = 1, HRX_VERIFY_ENABLE = 2, HRX_VERIFY_TRANSITION = 4, HRX_VERIFY_START_LOOKUP = 8, HRX_VERIFY_END_LOOKUP = 16,
       HRX_VERIFY_ACCEPT = 32, HRX_VERIFY_FLAGS = 64, HRX_VERIFY_PADDING = 128, HRX_VERIFY_MASK = 256,
       HRX_VERIFY_CIRCUIT_BITS = 63, HRX_VERIFY_ROW_SHIFT = 32 };
int hrx_verify_rows_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                           const uint32_t *records, size_t rec_pitch, const uint16_t *masked, size_t msk_pitch,
                           size_t B, size_t M, uint64_t *verdict, void *stream);
int hrx_verify_rows_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                                  const uint32_t *const *record_planes, size_t n_planes, const uint16_t *masked,
                                  size_t B, size_t M, uint64_t *verdict, void *stream);
/* The same rules over rows in HOST memory (as hrx_witness_columns_host takes them: string-major with pitches, or position-major as copied from the
 * device), on a host-only or a device context, over HRX_OPT_HOST_THREADS threads by ranges of strings.  The definition of the verdict word. */
int hrx_verify_rows_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                         const uint32_t *records, size_t rec_pitch, const uint16_t *masked, size_t msk_pitch,
                         size_t B, size_t M, uint64_t *verdict);
/* CHUNKED VERIFY — the same verdict words, bit for bit, with every string's rows cut into chunks of `chunk_rows` rows so that few long strings fill
 * the device (one lane per string leaves 8192 x 32768 on an eighth of the SIMDs).  A first launch judges every (64 strings, chunk) pair on its own
 * and leaves a summary of eight u32 words per (string, chunk) in the caller's workspace; a second launch folds each string's summaries in row order
 * into the verdict word.  No atomics, no context scratch, nothing allocated, no synchronisation; deterministic; capturable under the first-call rule
 * above.  chunk_rows: a multiple of 32, or 0 = hrx_ctx_verify_chunk_rows(ctx, B, M); a value of M or more is one chunk.
 * hrx_verify_chunked_workspace_bytes: what a call with this chunk_rows needs (32 bytes x ceil(M / chunk_rows) x B; 0: chunk_rows is 0 or no
 * multiple of 32, or the shape is out of range).  Context-free. */
size_t hrx_verify_chunked_workspace_bytes(size_t B, size_t M, size_t chunk_rows);
/* The context's pick for a shape: the fewest chunks that give every SIMD of its device two waves (256 CUs on a host-only context), but no more than
 * M / 256 of them (no chunk below 256 rows; measured: DESIGN.md §17), the rows cut evenly in multiples of 64.  A value >= M means one chunk: hrx_verify_rows_device is the better call.  0: NULL ctx. */
size_t hrx_ctx_verify_chunk_rows(hrx_ctx *ctx, size_t B, size_t M);
/* Stands in for hrx_verify_rows_device: its arguments, with chunk_rows and the workspace (device memory, 16-byte aligned, at least
 * hrx_verify_chunked_workspace_bytes(B, M, chunk_rows) bytes — for chunk_rows = 0 of the context's pick; its contents before the call do not matter
 * and it is free again once the call's work on `stream` is done) before verdict.  Two launches, asynchronous on `stream`.  Refused with HRX_ERR_ARG,
 * nothing written: whatever hrx_verify_rows_device refuses, chunk_rows no multiple of 32, a NULL or misaligned or too small workspace, more than
 * 2^31 - 1 (64 strings, chunk) pairs.  A host-only context: HRX_ERR_HIP. */
int hrx_verify_rows_chunked_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                                   const uint32_t *records, size_t rec_pitch, const uint16_t *masked, size_t msk_pitch,
                                   size_t B, size_t M, size_t chunk_rows, void *workspace, size_t workspace_bytes,
                                   uint64_t *verdict, void *stream);
/* Stands in for hrx_verify_rows_device_planes in the same way. */
int hrx_verify_rows_chunked_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                                          const uint32_t *const *record_planes, size_t n_planes, const uint16_t *masked,
                                          size_t B, size_t M, size_t chunk_rows, void *workspace, size_t workspace_bytes,
                                          uint64_t *verdict, void *stream);
/* Stands in for hrx_verify_rows_host: the same chunk walk and fold (csrc/hrx_verify.hpp) on HRX_OPT_HOST_THREADS threads over (string, chunk)
 * pairs, so eight long strings use sixteen threads.  The summaries are the call's own allocation.  The definition of the chunked rule. */
int hrx_verify_rows_chunked_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                                 const uint32_t *records, size_t rec_pitch, const uint16_t *masked, size_t msk_pitch,
                                 size_t B, size_t M, size_t chunk_rows, uint64_t *verdict);

/* ------------------------------------------------------------------ */
/* LOOKUP COUNTS — how often the advice rows hit each row of the fixed lookup tables (the first step of a prover over the cells)      */
/* ------------------------------------------------------------------ */
/* RegexVerifyConfig::configure declares three lookups per RegexDefs (src/lib.rs:206-285): "characters and their state" into the transition table,
 * "start_state of substring" and "end_state of substring" into the endpoint table.  For each of them and each table row, in RegexTableConfig::load's
 * order (hrx_table_transition_rows / hrx_table_endpoint_rows: T_d and E_d rows of def d), these calls count the rows of a string's witness that look
 * that table row up: the multiplicity column m of a logUp-style argument, and what halo2's own lookup argument builds its permuted columns A', S'
 * from (table row t, m[t] times) without a sort.  Per row r of the M rows, with en = [r < n_b], se / ee the record's start_enable / end_enable bits
 * and next = the state of row r + 1 (the def's dummy state behind row M - 1):
 *   trans  (en char, en cur + (1 - en) dummy, en next + (1 - en) dummy, en substr_id)     lib.rs:218-232
 *   start  (se substr_id, se cur + (1 - se) dummy, dummy)                                   lib.rs:247-257
 *   end    (ee substr_id, dummy, ee next + (1 - ee) dummy)                                  lib.rs:273-283
 * each adds 1 to the table row that equals it in every component — the lowest such row where two endpoint rows hold one tuple — or, in no row, 1 to the
 * string's `misses` word and to no bin: misses[b] != 0 exactly where hrx_verify_rows_host reports a transition, start or end lookup bit.  The lookups
 * that exist are those VERIFY judges: with n_b == M the transition and end lookups of row M - 1 read a cell match_substrs never assigns and are neither
 * counted nor missed.  States, ids and flag bits outside every table are misses.  n_b > M: every bin 0, misses 0xffffffff.  No status word is read:
 * rows are counted as they lie.
 * counts: [b_count][W] u32, 16-byte aligned, W = hrx_lookup_words_per_string(defs): per def in order trans[T_d], start[E_d], end[E_d], the total rounded
 * up to a multiple of 4 with the pad words written as 0; hrx_lookup_layout gives one def's offsets into a string's run.  misses: [b_count] u32, or NULL.
 * The strings are [b_begin, b_begin + b_count) of the batch, as for hrx_fr_columns_device (the dense output is large: the caller bounds it).
 * `layout`, chars / stride / lens, records (rec_pitch string-major only, in rows; 0 = M) and the record planes are those of hrx_verify_rows_device*, at
 * its alignments; whatever it refuses is refused, and a refused call writes nothing.  The masked rows are no argument: no lookup reads them.
 * The device forms: one launch, asynchronous on `stream`; nothing allocated, no context scratch, no global atomics, deterministic.  The image of the
 * tables is built and uploaded at the context's FIRST lookup call: inside a stream capture before that HRX_ERR_STATE, afterwards capturable.  A
 * host-only context: HRX_ERR_HIP. */
size_t hrx_lookup_words_per_string(const hrx_defs *defs);
int hrx_lookup_layout(const hrx_defs *defs, size_t def, size_t *trans_off, size_t *trans_rows, size_t *start_off, size_t *end_off, size_t *endpoint_rows);
int hrx_lookup_counts_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                             const uint32_t *records, size_t rec_pitch, size_t B, size_t M, size_t b_begin, size_t b_count,
                             uint32_t *counts, uint32_t *misses, void *stream);
int hrx_lookup_counts_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                                    const uint32_t *const *record_planes, size_t n_planes, size_t B, size_t M, size_t b_begin, size_t b_count,
                                    uint32_t *counts, uint32_t *misses, void *stream);
/* The same over rows in HOST memory (as hrx_verify_rows_host takes them), on a host-only or a device context, over HRX_OPT_HOST_THREADS threads by
 * ranges of strings.  The definition of the counts. */
int hrx_lookup_counts_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                           const uint32_t *records, size_t rec_pitch, size_t B, size_t M, size_t b_begin, size_t b_count,
                           uint32_t *counts, uint32_t *misses);
/* How a device call of b_count strings cuts its work: a workgroup keeps the bins of *group consecutive strings of the window in LDS (a power of two,
 * chosen from W and lowered while fewer than two workgroups per CU would come of it; 256 CUs on a host-only context) and walks the rows *passes times
 * (more than once only where one string's bins exceed the LDS of a CU).  For tests and tools; the counts do not depend on it. */
int hrx_ctx_lookup_group(hrx_ctx *ctx, size_t b_count, size_t *group, size_t *passes);

/* ------------------------------------------------------------------ */
/* LOOKUP COMPRESS — the lookup tuples folded with a challenge into field cells (what the counts above are indices into)                  */
/* ------------------------------------------------------------------ */
/* A lookup argument does not work on tuples but on the tuple folded with the challenge theta: for the input expressions [e0 .. ek-1] of meta.lookup halo2's
 * commit_permuted computes acc = acc * theta + e_i from 0 — A = e0 theta^3 + e1 theta^2 + e2 theta + e3 for the transition lookup, e0 theta^2 + e1 theta + e2
 * for the two endpoint lookups — and folds the table columns the same way into S.  These calls compute both sides in bn256::Fr, so that with the counts the
 * first phase of either lookup argument is gathers only: A'[i] = S[a_idx[i]] with the indices of a sort-free permutation of the counts, m = the counts.
 *
 * INPUTS.  cells: [3 D][b_count][M][4] u64 in hrx_fr_columns_device's shape (hrx_lookup_num_columns(D) = 3 D columns), 16-byte aligned; column 3 d + k
 * holds k = 0 the transition, 1 the start, 2 the end lookup of def d; the strings are [b_begin, b_begin + b_count).  The tuples are those of LOOKUP COUNTS,
 * as integers, and nothing is left out: with n_b == M the transition and end cells of row M - 1 are computed from next = the dummy state like any other (the
 * cell match_substrs never assigns).  Values are folded as they lie: a state, id or flag outside every table is folded as the integer the record holds, so
 * a tampered row's cell is in no table row.  n_b > M: the string has no rows, every limb of every one of its cells is 0.
 * theta: 4 u64 limbs per challenge, 8-byte aligned, in DEVICE memory for the device forms (a transcript running on the device can write it, and the call
 * stays capturable); theta_stride in u64 words: 4 — theta[4 i] is the challenge of string b_begin + i; 0 — one for the whole call; anything else
 * HRX_ERR_ARG.  The limbs are taken mod r first.  flags: 0 — theta and the cells are Montgomery limbs (x * 2^256 mod r, the in-memory form of Fr); or
 * HRX_FR_CANONICAL — both are plain integers; other bits HRX_ERR_ARG.
 * `layout`, chars / stride / lens, records (rec_pitch) and the record planes are those of hrx_lookup_counts_device*: whatever it refuses is refused, and a
 * refused call writes nothing.  The device forms: one launch (per 32768 strings), asynchronous on `stream`; nothing allocated, no context scratch, no
 * atomics, deterministic; no image of the tables is read, so they are capturable from the first call.  A host-only context: HRX_ERR_HIP. */
size_t hrx_lookup_num_columns(size_t D);
int hrx_lookup_compress_inputs_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                                      const uint32_t *records, size_t rec_pitch, size_t B, size_t M, size_t b_begin, size_t b_count,
                                      const uint64_t *theta, size_t theta_stride, uint64_t *cells, int flags, void *stream);
int hrx_lookup_compress_inputs_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                                             const uint32_t *const *record_planes, size_t n_planes, size_t B, size_t M, size_t b_begin, size_t b_count,
                                             const uint64_t *theta, size_t theta_stride, uint64_t *cells, int flags, void *stream);
/* The same over rows, theta and cells in HOST memory, on a host-only or a device context, over HRX_OPT_HOST_THREADS threads by ranges of strings.  The
 * definition of the cells. */
int hrx_lookup_compress_inputs_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens,
                                    const uint32_t *records, size_t rec_pitch, size_t B, size_t M, size_t b_begin, size_t b_count,
                                    const uint64_t *theta, size_t theta_stride, uint64_t *cells, int flags);
/* TABLE.  cells: [n_theta][W][4] u64, 16-byte aligned, W = hrx_lookup_words_per_string(defs), in the index space of the counts: cell w of a run is the
 * compressed table row that counts[w] counts.  trans[T_d]: the fold of (char, cur, next, substr_id) of transition row t; start[E_d] and end[E_d]: both the
 * fold of (substr_id, start_state, end_state) of endpoint row e — the two lookups share the endpoint table's columns, the runs hold equal cells and the
 * indices stay those of hrx_lookup_layout; the pad words are zero cells.  Run t is folded with theta[t * theta_stride] (theta, theta_stride and flags as
 * above; n_theta at most 65535).  The rows are those RegexTableConfig::load assigns, never a walk's table; their flat tuple array is built — and for the
 * device form uploaded — at the context's FIRST call of this kind: inside a stream capture before that HRX_ERR_STATE, afterwards one launch, capturable. */
int hrx_lookup_compress_table_device(hrx_ctx *ctx, const uint64_t *theta, size_t theta_stride, size_t n_theta, uint64_t *cells, int flags, void *stream);
int hrx_lookup_compress_table_host(hrx_ctx *ctx, const uint64_t *theta, size_t theta_stride, size_t n_theta, uint64_t *cells, int flags);
/* The Montgomery product a * b / 2^256 mod r on the host (the kernels' arithmetic): Montgomery limbs of two elements below r in, Montgomery limbs out. */
void hrx_fr_mul(const uint64_t *a, const uint64_t *b, uint64_t *out);

/* ------------------------------------------------------------------ */
/* LOOKUP PERMUTE — the permuted columns A', S' of halo2's lookup argument out of the counts, without a sort                                */
/* ------------------------------------------------------------------ */
/* halo2's prover (lookup::prover::commit_permuted) commits for every lookup to a permutation A' of the compressed inputs and a permutation S' of the
 * compressed table with A'[0] = S'[0] and, for every row i, A'[i] = S'[i] or A'[i] = A'[i - 1].  Any such pair is a valid witness; these calls build one
 * from the counts alone, for every lookup of every string of a window, as indices and — optionally — as cells gathered from the compressed table.
 * The rule, for one lookup with a table of T rows (T_d or E_d of hrx_lookup_layout), its counts m[0 .. T) in the string's run and n_rows usable rows:
 *   sum = the sum of m[t], in 64 bits; sum > n_rows: the lookup OVERFLOWS (below).  Otherwise m'[0] = m[0] + (n_rows - sum), m'[t] = m[t] elsewhere:
 *   the circuit's rows that no row of the string covers evaluate to the tables' first row, the dummy tuple.  A_idx is non-decreasing and holds row t
 *   m'[t] times.  Position i is a first position where i == 0 or A_idx[i] != A_idx[i - 1]; there S_idx[i] = A_idx[i].  The j-th position (from 0) that is
 *   no first position takes the j-th element of the fill list: the rows with m'[t] == 0 ascending, then row 0 n_rows - T times (the table padded to the
 *   circuit's rows with copies of its first row).
 * counts: [b_count][W] u32 exactly as hrx_lookup_counts_device writes them, 16-byte aligned.  `misses` is no argument: the columns are built from the
 * counts as they lie, and a caller who wants a valid argument checks misses == 0 itself.  M is no argument either: rows beyond a string's own are the
 * n_rows - sum rows of row 0.  With n_b == M the counts leave the transition and end lookups of row M - 1 out (LOOKUP COUNTS), so in A' those two inputs
 * appear as the dummy row's cell, not as the cell hrx_lookup_compress_inputs_device computes for that row.
 * n_rows: at least every T_d and E_d of the defs, at most 2^24.  pitch: the entries between consecutive (column, string) runs of the outputs, at least
 * n_rows and a multiple of 4 (a caller passes 2^k to write straight into polynomial buffers); 0 = n_rows rounded up to a multiple of 4.  Entries
 * [n_rows, pitch) are never written: the blinding rows are the caller's.
 * a_idx, s_idx: [3 D][b_count][pitch] u32, 16-byte aligned, column 3 d + k in hrx_lookup_num_columns' order (k = 0 trans, 1 start, 2 end); the entries are
 * word indices into the string's run — trans_off + t, start_off + e, end_off + e: the index space of the counts and of hrx_lookup_compress_table_device.
 * Both or neither.  a_cells, s_cells: [3 D][b_count][pitch][4] u64, 16-byte aligned: the table cell at the index, copied limb for limb (Montgomery and
 * canonical limbs alike; no arithmetic).  table_cells: [runs][W][4] u64 as hrx_lookup_compress_table_device writes it, 16-byte aligned; table_stride in
 * u64 words: 0 — one run for the whole call; 4 W — run i belongs to string i of the window; anything else HRX_ERR_ARG.  All three or none; at least one
 * of the index pair and the cell pair.
 * overflow: [b_count] u32 or NULL (at most 10 defs with it): bit 3 d + k is set where that lookup's sum exceeds n_rows.  Of such a lookup every index in
 * [0, n_rows) is 0xffffffff and every limb of its cells 0; the string's other lookups are not affected.  No count value ever forms an address.
 * Refused with HRX_ERR_ARG, nothing written: NULL counts, half-given pairs or no output, misaligned buffers, a bad table_stride, n_rows or pitch, and for
 * the device form a missing, misaligned (256 bytes) or too small workspace.  A host-only context: HRX_ERR_HIP for the device form.
 * The device form: one launch, one more with `overflow`, asynchronous on `stream`; nothing allocated, no context scratch, no global atomics,
 * deterministic; no image of the tables is read, so it is capturable from a context's first call.  workspace: device memory of
 * hrx_lookup_permute_workspace_bytes(defs, b_count, n_rows) bytes — 0, and NULL accepted, unless a table of the defs has more rows than the kernel keeps
 * in LDS at once (its lists of empty rows then lie there); its contents do not matter and it is free again once the call's work on `stream` is done. */
size_t hrx_lookup_permute_workspace_bytes(const hrx_defs *defs, size_t b_count, size_t n_rows);
int hrx_lookup_permute_device(hrx_ctx *ctx, const uint32_t *counts, size_t b_count, size_t n_rows, size_t pitch,
                              uint32_t *a_idx, uint32_t *s_idx,
                              const uint64_t *table_cells, size_t table_stride, uint64_t *a_cells, uint64_t *s_cells,
                              uint32_t *overflow, void *workspace, size_t workspace_bytes, void *stream);
/* The same with everything in HOST memory, on a host-only or a device context, over HRX_OPT_HOST_THREADS threads by ranges of strings.  The definition
 * of the columns. */
int hrx_lookup_permute_host(hrx_ctx *ctx, const uint32_t *counts, size_t b_count, size_t n_rows, size_t pitch,
                            uint32_t *a_idx, uint32_t *s_idx,
                            const uint64_t *table_cells, size_t table_stride, uint64_t *a_cells, uint64_t *s_cells,
                            uint32_t *overflow);
/* How a device call cuts its work: a workgroup serves one (string, lookup) and *group_rows positions of it (*groups workgroups per lookup: 1 unless the
 * window is too small to fill the device), expands them *tile_rows positions at a time on absolute tile borders, and walks the table *chunk_rows rows at
 * a time (a table of more rows: one workgroup per lookup, and a workspace).  For tests and tools; the columns do not depend on it. */
int hrx_ctx_lookup_permute_plan(hrx_ctx *ctx, size_t b_count, size_t n_rows, size_t *tile_rows, size_t *chunk_rows, size_t *group_rows, size_t *groups);

/* ------------------------------------------------------------------ */
/* LOOKUP PRODUCT — the grand product Z of halo2's lookup argument, its denominators from inverse tables                                      */
/* ------------------------------------------------------------------ */
/* The last column of lookup::prover (commit_permuted, then commit_product): Z[0] = 1, Z[i + 1] = Z[i] (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] +
 * gamma)).  A' and S' are table cells selected by the index columns of LOOKUP PERMUTE, so both inversions are needed per TABLE row, not per witness row:
 * with a table of 1 / (S + beta) and one of 1 / (S + gamma) a row's term is three multiplications and two gathers, and Z is a running product.  All
 * arithmetic is in bn256::Fr; cells are 4 u64 limbs, Montgomery by default and plain integers with HRX_FR_CANONICAL in `flags` (other bits HRX_ERR_ARG), as
 * in LOOKUP COMPRESS; every cell written is a fully reduced element, so the device forms equal the host forms limb for limb.  Every table, input and
 * inverse cell read must be below r — every producer in this library writes such cells; the sums S + shift, A + beta and S + gamma add the cells as they
 * are, and a cell of r or more can leave a sum unreduced there — and only `shift`, `beta` and `gamma` are reduced by the calls.
 *
 * INVERSE TABLE (also what a logUp prover needs: m / (S + beta) directly, 1 / (A + beta) by gather).  table_cells: [n_runs][W][4] u64 as
 * hrx_lookup_compress_table_* writes it, W = hrx_lookup_words_per_string(defs); shift: 4 u64 limbs per run, 8-byte aligned, in DEVICE memory for the device
 * form, taken mod r first; shift_stride in u64 words: 4 — shift[4 t] belongs to run t; 0 — one for the call; anything else HRX_ERR_ARG.
 * inv_cells: [n_runs][W][4] u64: inv[w] = (S[w] + shift)^-1, or the zero cell where S[w] + shift = 0 (halo2's batch_invert: zeros stay zero); the pad words
 * of a run are written as zero cells.  Both cell buffers 16-byte aligned; they must not overlap.  The device form: ONE launch, a workgroup per run (batch
 * inversion: prefix products, one Fermat inversion x^(r - 2) per run by one lane, suffix products), asynchronous on `stream`; nothing allocated, no context
 * scratch, no atomics, deterministic; no image of the tables is read, so it is capturable from a context's first call.  workspace:
 * hrx_lookup_invert_workspace_bytes(defs, n_runs) bytes of device memory, 256-byte aligned — 0 in this build, and NULL accepted (a build that moves the
 * Fermat step into a launch of its own keeps the runs' totals there); a misaligned or too small one is refused.
 *
 * PRODUCT, for every lookup c = 3 d + k (hrx_lookup_num_columns' order) of every string b_begin + i, i < b_count, of a batch whose lengths are lens (the
 * whole batch's array) and whose rows are M: with (off, T) the lookup's words in the string's run (hrx_lookup_layout) and rows r = 0 .. n_rows - 1,
 *   A[r]    = in_cells' cell of row r for r < M, the lookup's dummy cell table[off] for r >= M — and where the counts leave an input out, so that A and A'
 *             stay one multiset: with n_b == M row M - 1 of the transition and the end lookup; with n_b > M every row
 *   S[r]    = table[off + r] for r < T, table[off] for r >= T (LOOKUP PERMUTE's padding)
 *   term[r] = 0 where a_idx[r] or s_idx[r] lies outside [off, off + T) — LOOKUP PERMUTE's overflow pattern 0xffffffff included; no index is used as an
 *             address before that test — else (A[r] + beta)(S[r] + gamma) inv_beta[a_idx[r]] inv_gamma[s_idx[r]]
 *   Z[0] = 1, Z[r + 1] = Z[r] term[r]: entries [0, n_rows] of the lookup's column are written (halo2's z over the usable rows and the row of l_last);
 *   entries above n_rows never: the blinding rows are the caller's.
 * open: [b_count] u32 or NULL (at most 10 defs with it): bit 3 d + k is set where Z[n_rows] != 1.  A zero term keeps Z zero from there on, so a bad index or
 * a zero denominator always ends in `open`; there is no other error path.
 * in_cells: [3 D][b_count][M][4] u64 as hrx_lookup_compress_inputs_* writes them; a_idx, s_idx: [3 D][b_count][idx_pitch] u32 as hrx_lookup_permute_*
 * writes them (idx_pitch: a multiple of 4, at least n_rows; 0 = n_rows rounded up); table_cells, inv_beta, inv_gamma: [runs][W][4] u64 with ONE
 * table_stride: 0 — one run for the call; 4 W — run i belongs to string i of the window; beta, gamma: 4 u64 limbs each, as `shift` above, with
 * challenge_stride 4 (per string of the window) or 0; n_rows: LOOKUP PERMUTE's bounds.  z: [3 D][b_count][z_pitch][4] u64; z_pitch: a multiple of 4 above
 * n_rows (2^k to write straight into polynomial buffers); 0 = n_rows + 1 rounded up.  Cells, index columns and tables 16-byte aligned.
 * Refused with HRX_ERR_ARG, nothing written: NULL inputs, misaligned buffers, strides other than those named, n_rows or a pitch out of range, unknown flag
 * bits.  A host-only context: HRX_ERR_HIP for the device forms.
 * The device form: one launch, one more with `open` (one wave per string: a word has one writer), asynchronous on `stream`; nothing allocated, no context
 * scratch, no atomics, deterministic; capturable from a context's first call.  One workgroup serves a (string, lookup) from row 0 to n_rows: a window with
 * fewer lookups than the device has compute units is slow, not wrong. */
size_t hrx_lookup_invert_workspace_bytes(const hrx_defs *defs, size_t n_runs);
int hrx_lookup_invert_table_device(hrx_ctx *ctx, const uint64_t *table_cells, size_t n_runs, const uint64_t *shift, size_t shift_stride,
                                   uint64_t *inv_cells, int flags, void *workspace, size_t workspace_bytes, void *stream);
int hrx_lookup_product_device(hrx_ctx *ctx, const uint32_t *lens, size_t M, size_t b_begin, size_t b_count,
                              const uint64_t *in_cells, const uint32_t *a_idx, const uint32_t *s_idx, size_t n_rows, size_t idx_pitch,
                              const uint64_t *table_cells, const uint64_t *inv_beta, const uint64_t *inv_gamma, size_t table_stride,
                              const uint64_t *beta, const uint64_t *gamma, size_t challenge_stride,
                              uint64_t *z, size_t z_pitch, uint32_t *open, int flags, void *stream);
/* The same with everything in HOST memory, on a host-only or a device context, over HRX_OPT_HOST_THREADS threads by ranges of runs and of strings.  The
 * definition of the cells. */
int hrx_lookup_invert_table_host(hrx_ctx *ctx, const uint64_t *table_cells, size_t n_runs, const uint64_t *shift, size_t shift_stride,
                                 uint64_t *inv_cells, int flags);
int hrx_lookup_product_host(hrx_ctx *ctx, const uint32_t *lens, size_t M, size_t b_begin, size_t b_count,
                            const uint64_t *in_cells, const uint32_t *a_idx, const uint32_t *s_idx, size_t n_rows, size_t idx_pitch,
                            const uint64_t *table_cells, const uint64_t *inv_beta, const uint64_t *inv_gamma, size_t table_stride,
                            const uint64_t *beta, const uint64_t *gamma, size_t challenge_stride,
                            uint64_t *z, size_t z_pitch, uint32_t *open, int flags);
/* How a device product call cuts its work: a workgroup walks its lookup's Z column *tile_rows entries at a time, *rows_per_lane consecutive entries per
 * lane, one workgroup per (string, lookup) whatever the window.  For tests and tools; the cells do not depend on it. */
int hrx_ctx_lookup_product_plan(hrx_ctx *ctx, size_t b_count, size_t n_rows, size_t *tile_rows, size_t *rows_per_lane);

/* ------------------------------------------------------------------ */
/* FR NTT — columns of field cells to coefficients and to cosets: the transform of size 2^k over bn256::Fr                                    */
/* ------------------------------------------------------------------ */
/* What halo2 does next with every Lagrange column the lookup stages write — lagrange_to_coeff, coeff_to_extended, extended_to_coeff — is one batched
 * number-theoretic transform.  The two-adic subgroup is halo2curves': S = 28, generator 7, ROOT_OF_UNITY = 7^((r - 1) / 2^28) =
 * 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c, w_k = ROOT_OF_UNITY^(2^(28 - k)).  For every column x[0 .. 2^k) of n_cols, natural
 * order in and out:
 *   forward (default):          y[j] = sum_i (g^i x[i]) w_k^(i j)
 *   inverse (HRX_NTT_INVERSE):  y[i] = g^i 2^-k sum_j x[j] w_k^(-i j)
 * g is `shift`: 4 u64 limbs in the call's limb form, 8-byte aligned, taken mod r first, in DEVICE memory for the device form; NULL: g = 1, and no
 * multiplications are spent on it.  The call never inverts g: a forward transform with g is undone by the inverse with g^-1.
 *   lagrange_to_coeff: inverse, no shift.  coeff_to_extended: forward at the extended k, n_in = 2^k of the column, shift = the coset generator.
 *   extended_to_coeff: inverse with the generator's inverse.
 * in: [n_cols][in_pitch][4] u64, entries [0, n_in) of a column are read, 1 <= n_in <= 2^k, entries [n_in, 2^k) count as zero and are NEVER read (halo2's
 * zero extension without clearing memory); out: [n_cols][out_pitch][4] u64, entries [0, 2^k) of a column are written, entries above never.  Pitches in
 * cells, multiples of 4, in_pitch >= n_in, out_pitch >= 2^k; both buffers 16-byte aligned.  in == out with equal pitches is the in-place form; any other
 * overlap of the two ranges is refused.  1 <= k <= 24.  Cells are Montgomery limbs by default, plain integers with HRX_FR_CANONICAL (the transform is
 * linear: the flag changes how `shift` is read and nothing per cell).  Every input cell read must be below r — every producer in this library writes such
 * cells; unshifted, the first butterfly adds the cells as they are, and a cell of r or more can lose a carry there — and only `shift` is reduced by the call.
 * Every cell written is a fully reduced element: the device form equals the host form limb for limb.
 * workspace: hrx_fr_ntt_workspace_bytes(k) bytes of device memory, 256-byte aligned, written by hrx_fr_ntt_prepare_device in ONE launch (the table
 * w_k^e, e < 2^(k-1), each entry by square-and-multiply, and 2^-k) and read-only afterwards: it serves any number of transform calls of that k, on any
 * streams and contexts of the device.  Nothing depends on g in it.
 * The device form: asynchronous on `stream`; one launch for k <= 12 (a column in one workgroup's LDS, 2^(10 - k) columns per workgroup below k = 10), else
 * one permuting launch and one per pass (hrx_ctx_fr_ntt_plan) — a fixed number given k; no atomics, nothing allocated, no context state, deterministic;
 * capturable from a context's first call.
 * Refused with HRX_ERR_ARG, nothing written: NULL or misaligned buffers, k, n_in or a pitch out of range, a partial overlap, unknown flag bits, a missing,
 * misaligned or too small workspace.  A host-only context: HRX_ERR_HIP for the device forms.  n_cols == 0 launches nothing. */
enum { HRX_NTT_INVERSE = 2 };   /* beside HRX_FR_CANONICAL in `flags` */
size_t hrx_fr_ntt_workspace_bytes(unsigned k);   /* 0 for a k out of range */
int hrx_fr_ntt_prepare_device(hrx_ctx *ctx, unsigned k, void *workspace, size_t workspace_bytes, void *stream);
int hrx_fr_ntt_device(hrx_ctx *ctx, const uint64_t *in, size_t in_pitch, uint64_t *out, size_t out_pitch, size_t n_cols, unsigned k, size_t n_in,
                      const uint64_t *shift, int flags, const void *workspace, size_t workspace_bytes, void *stream);
/* The same with everything in HOST memory, on a host-only or a device context: an iterative radix-2 transform per column over HRX_OPT_HOST_THREADS threads
 * by ranges of columns; it computes its own twiddles and takes no workspace.  The definition of the cells. */
int hrx_fr_ntt_host(hrx_ctx *ctx, const uint64_t *in, size_t in_pitch, uint64_t *out, size_t out_pitch, size_t n_cols, unsigned k, size_t n_in,
                    const uint64_t *shift, int flags);
/* How a device call cuts its work: *n_passes passes of pass_bits[0 .. *n_passes) butterfly stages each (pass_bits: room for 3; the unused ones 0), their sum
 * k; one pass: the call is one launch and a workgroup takes *cols_per_group whole columns; more: a permuting launch, then a launch per pass.  For tests and
 * tools; the cells do not depend on it. */
int hrx_ctx_fr_ntt_plan(hrx_ctx *ctx, size_t n_cols, unsigned k, size_t *n_passes, size_t *pass_bits, size_t *cols_per_group);
/* out = a - b mod r on 4-limb values of one form, each taken mod r first (beside hrx_fr_mul: for tests and bindings) */
void hrx_fr_sub(const uint64_t *a, const uint64_t *b, uint64_t *out);

/* ------------------------------------------------------------------ */
/* LOOKUP QUOTIENT — the lookup argument's five constraints on the extended coset, folded into the quotient and divided by X^n - 1                */
/* ------------------------------------------------------------------ */
/* What halo2 does with the columns FR NTT takes to the extended coset: the lookup part of evaluate_h.  n = 2^k, e = ext_k - k, N = 2^ext_k, rot = 2^e; point
 * j of the extended coset is g w_ext^j, so p(w X) at point j is p at point (j + rot) mod N and p(w^-1 X) is p at point (j - rot) mod N.  For every string
 * i < b_count, lookups c = 0 .. 3 D - 1 in hrx_lookup_num_columns' order, every point j < N, with v = h_in[j] (0 where h_in is NULL, and then it is never
 * read), every lookup applies halo2's five steps in halo2's order:
 *   v = v y + (1 - Z[j]) l0[j]
 *   v = v y + (Z[j]^2 - Z[j]) l_last[j]
 *   v = v y + (Z[j + rot] (A'[j] + beta) (S'[j] + gamma) - Z[j] (A[j] + beta) (S[j] + gamma)) l_active[j]
 *   v = v y + (A'[j] - S'[j]) l0[j]
 *   v = v y + (A'[j] - S'[j]) (A'[j] - A'[j - rot]) l_active[j]
 * and h_out[j] = v after the last lookup — v t_inv[j mod rot] with HRX_QUOTIENT_DIVIDE in `flags`.  The implementations regroup the steps (powers of y, the
 * expressions grouped by selector: 12 products a lookup and point instead of 16); every cell written is a fully reduced element, so the device form equals
 * the host form limb for limb.  Cells are Montgomery limbs by default, plain integers with HRX_FR_CANONICAL; the expressions are not linear in the cells,
 * and what the plain form costs is paid per point and string, not per cell (csrc/hrx_quotient.hpp).  Every cell read must be below r; only beta, gamma and y
 * are reduced by the call.
 * a_ext, ap_ext, sp_ext, z_ext: [3 D][b_count][pitch][4] u64, the compressed inputs A, the permuted columns A', S' and the grand product Z on the extended
 * coset (hrx_fr_ntt_* at ext_k with the coset's generator as shift).  s_ext: [3 D][runs][s_pitch][4], the compressed table S the same way; s_stride 0 — one
 * run for the call; 1 — run i belongs to string i of the window; anything else HRX_ERR_ARG.  selectors: [3][sel_pitch][4] — l0, the Lagrange basis
 * polynomial of row 0; l_last, that of row n_rows (LOOKUP PERMUTE's and LOOKUP PRODUCT's n_rows: Z's entries [0, n_rows] are the ones the product call
 * writes); l_active, the sum of the bases of rows [0, n_rows) — on the same coset.  beta, gamma, y: 4 u64 limbs each, 8-byte aligned, in DEVICE memory for
 * the device form, taken mod r first; challenge_stride in u64 words, one for the three: 4 — per string of the window; 0 — one set for the call.
 * h_in, h_out: [b_count][h_pitch][4]; h_in NULL, or == h_out (in place), or apart from it; h_out apart from every input.  Entries [0, 2^ext_k) of every
 * h_out column are written and none above; no input is written.  Pitches in cells, multiples of 4, at least 2^ext_k; cell buffers 16-byte aligned.
 * 1 <= k, 1 <= ext_k - k <= 6, ext_k <= 24.  t_inv: [2^(ext_k - k)][4], required with HRX_QUOTIENT_DIVIDE and ignored otherwise.
 * VANISHING INVERSE.  t_inv[c] = 1 / (g^n w_ext^(n c) - 1), c < 2^(ext_k - k): the values X^n - 1 takes on the coset, inverted; the zero cell where that is
 * zero (g in the subgroup), as in hrx_lookup_invert_table_*.  g is `shift` as FR NTT reads it (the call's limb form, taken mod r first, DEVICE memory for the
 * device form; NULL: g = 1, where entry 0 is the zero cell).  Once per (k, ext_k, g): one launch of one workgroup, a lane per entry.
 * Refused with HRX_ERR_ARG, nothing written: NULL or misaligned buffers, k, ext_k, a pitch or a stride out of range, an overlap other than h_in == h_out,
 * HRX_QUOTIENT_DIVIDE without t_inv, unknown flag bits.  A host-only context: HRX_ERR_HIP for the device forms.
 * The device form: ONE launch, asynchronous on `stream`; a workgroup takes a tile of consecutive points of one string and carries v in registers across
 * all 3 D lookups; nothing allocated, no context scratch, no atomics, no grid-wide barrier, deterministic; capturable from a context's first call.
 * b_count == 0 launches nothing. */
enum { HRX_QUOTIENT_DIVIDE = 4 };   /* beside HRX_FR_CANONICAL in `flags` */
int hrx_fr_vanishing_inverse_device(hrx_ctx *ctx, unsigned k, unsigned ext_k, const uint64_t *shift, uint64_t *t_inv, int flags, void *stream);
int hrx_lookup_quotient_device(hrx_ctx *ctx, size_t b_count, unsigned k, unsigned ext_k,
                               const uint64_t *a_ext, const uint64_t *ap_ext, const uint64_t *sp_ext, const uint64_t *z_ext, size_t pitch,
                               const uint64_t *s_ext, size_t s_pitch, size_t s_stride, const uint64_t *selectors, size_t sel_pitch,
                               const uint64_t *beta, const uint64_t *gamma, const uint64_t *y, size_t challenge_stride,
                               const uint64_t *h_in, uint64_t *h_out, size_t h_pitch, const uint64_t *t_inv, int flags, void *stream);
/* The same with everything in HOST memory, on a host-only or a device context, the quotient over HRX_OPT_HOST_THREADS threads by ranges of strings.  The
 * definition of the cells. */
int hrx_fr_vanishing_inverse_host(hrx_ctx *ctx, unsigned k, unsigned ext_k, const uint64_t *shift, uint64_t *t_inv, int flags);
int hrx_lookup_quotient_host(hrx_ctx *ctx, size_t b_count, unsigned k, unsigned ext_k,
                             const uint64_t *a_ext, const uint64_t *ap_ext, const uint64_t *sp_ext, const uint64_t *z_ext, size_t pitch,
                             const uint64_t *s_ext, size_t s_pitch, size_t s_stride, const uint64_t *selectors, size_t sel_pitch,
                             const uint64_t *beta, const uint64_t *gamma, const uint64_t *y, size_t challenge_stride,
                             const uint64_t *h_in, uint64_t *h_out, size_t h_pitch, const uint64_t *t_inv, int flags);
/* How a device quotient call cuts its work: a workgroup takes *tile_cells consecutive points of one string, *cells_per_lane per lane.  For tests and tools;
 * the cells do not depend on it. */
int hrx_ctx_lookup_quotient_plan(hrx_ctx *ctx, size_t b_count, unsigned ext_k, size_t *tile_cells, size_t *cells_per_lane);

/* ------------------------------------------------------------------ */
/* SURVEY §8 f3 — from the compact records to what the reference's fill consumes (host only, no context, re-entrant)   */
/* ------------------------------------------------------------------ */
/* One circuit: EXACTLY the Vecs the three derive_* calls at the top of match_substrs return (src/lib.rs:316-318), out of the string's compact records, so that the body
 * below lib.rs:318 runs unchanged on them (bindings/rust/hrx.rs WitnessOf is this call):
 *   records    [M][D] u32, string-major rows of ONE string (a row of hrx_witness_batch_host's output, or hrx_rows_of_string_position_major / _planes)
 *   n          characters.len() <= M
 *   states     [D][n + 1] u64   derive_states          (lib.rs:804-823); states[d][n] = the state after the last character
 *   substr_ids [D][n]     usize derive_substr_ids      (lib.rs:825-845)
 *   is_start   [D][n + 1] bool  derive_is_start_end.0  (lib.rs:847-888); is_start[d][n] = false
 *   is_end     [D][n + 1] bool  derive_is_start_end.1;                   is_end[d][0] = false
 * Exact: for i < n the enable cell is 1, so start_enable[i] = is_start[i] and end_enable[i] = is_end[i + 1] (lib.rs:482-519).  When n == M the records have no row n:
 * states[d][M] is returned as 0 and is_end[d][M] as false — the two values the reference computes and never assigns to a cell (lib.rs:388-418, 501).
 * Strings whose status word is not ok have no records to decode (the reference panics in derive_states, lib.rs:817). */
int hrx_witness_of_string(const uint32_t *records, size_t D, size_t n, size_t M, uint64_t *states, size_t *substr_ids, uint8_t *is_start, uint8_t *is_end);
/* All circuits of a batch, column-major: the integer content of every advice cell the loops of match_substrs assign (lib.rs:339-348 char_enable / characters,
 * 419-519 states / substr_ids / start_enable / end_enable per def) and of the two result columns (lib.rs:752-771), for strings [b_begin, b_begin + b_count) of a finished
 * batch that lies in HOST memory in `layout` (string-major with rec_pitch / msk_pitch in rows, 0 = M; or position-major as copied from the device):
 *   columns  [n_cols][b_count][M] u64, n_cols = hrx_witness_num_columns(D) = 4 + 4 D, in the column order of hrx_fr_columns_device:
 *            0 char_enable, 1 characters, 2+4d states[d], 3+4d substr_ids[d], 4+4d start_enable[d], 5+4d end_enable[d], 2+4D masked_characters, 3+4D all_substr_ids
 * — what `Value::known(F::from(v))` is applied to, one contiguous [M] run per circuit and column: a batch fill assigns them without a derive_* call or a gate evaluation per row. */
size_t hrx_witness_num_columns(size_t D);
int hrx_witness_columns_host(int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch, const uint16_t *masked,
                             size_t msk_pitch, size_t B, size_t M, size_t D, size_t b_begin, size_t b_count, uint64_t *columns);

/* ------------------------------------------------------------------ */
/* Multi-GPU driver for host buffers: strings are independent given the RegexDefs, so a batch shards by string index with
 * no collective.  One context per listed device (a device may be listed more than once: its shards then
 * run on separate streams); hrx_multi_witness_batch_host cuts the batch with hrx_shard_range, runs the shards
 * concurrently (one host thread per shard: staging copies and kernels of different devices overlap) and returns when
 * all are done.  Results are identical to one hrx_witness_batch_host call over the whole batch.  On error the first
 * failing shard's status is returned and hrx_last_error() tells which. */
typedef struct hrx_multi hrx_multi;
int hrx_multi_create(const hrx_defs *defs, const int *devices, int n_devices, hrx_multi **out);
void hrx_multi_destroy(hrx_multi *m);
int hrx_multi_num_shards(const hrx_multi *m);
int hrx_multi_shard_device(const hrx_multi *m, int shard);
int hrx_multi_witness_batch_host(hrx_multi *m, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M,
                                 uint32_t *records, uint16_t *masked, uint64_t *status);
/* Device-resident shards: the same driver without the PCIe copies, for a single-process host (the Rust prover) whose
 * inputs already sit in each device's HBM.  Shard r = counts[r] strings whose buffers chars[r], lens[r], records[r],
 * masked[r], status[r] are DEVICE pointers on the device of shard r (hrx_multi_shard_device), in `layout` (one of the
 * hrx_witness_batch_device_layout layouts, each shard a complete array of its own strings).  One kernel per shard is
 * enqueued on the shard's own stream — asynchronous; hrx_multi_synchronize waits for all of them.  No collective.
 * ORDERING: the shard streams are the contexts' private non-blocking streams; nothing orders them against the stream that
 * produced a shard's inputs.  The inputs must be complete before the call, or the caller makes the shard stream
 * (hrx_multi_shard_stream, a hipStream_t) wait on an event recorded behind the producer; the outputs are complete after
 * hrx_multi_synchronize (or behind an event recorded on the shard stream). */
void *hrx_multi_shard_stream(const hrx_multi *m, int shard);
int hrx_multi_witness_batch_device(hrx_multi *m, int layout, const uint8_t *const *chars, size_t stride, const uint32_t *const *lens,
                                   const size_t *counts, size_t M, uint32_t *const *records, uint16_t *const *masked,
                                   uint64_t *const *status);
int hrx_multi_synchronize(hrx_multi *m);

/* Contiguous shard [begin, begin+count) of a batch of B strings for `rank` of `world` devices
 * (strings are independent given the RegexDefs; no collective on the path). */
void hrx_shard_range(size_t B, int world, int rank, size_t *begin, size_t *count);

/* ------------------------------------------------------------------ */
/* Reference-shaped single-string entry points — src/lib.rs:804-888     */
/* ------------------------------------------------------------------ */
/* derive_states(&self, characters:&[u8]) -> Vec<Vec<u64>>: states[d*(n+1) + i].  On the reference's panic
 * returns HRX_ERR_INVALID_TRANSITION and hrx_last_error() is exactly
 * "The transition from {state} by {char} is invalid!" (lib.rs:817). */
int hrx_derive_states(hrx_ctx *ctx, const uint8_t *characters, size_t n, uint64_t *states);
/* derive_substr_ids(&self, states) -> Vec<Vec<usize>>: substr_ids[d*n + i] */
int hrx_derive_substr_ids(hrx_ctx *ctx, const uint64_t *states, size_t n, uint64_t *substr_ids);
/* derive_is_start_end(&self, states, substr_ids) -> (Vec<Vec<bool>>, Vec<Vec<bool>>): each [d*(n+1) + i] */
int hrx_derive_is_start_end(hrx_ctx *ctx, const uint64_t *states, const uint64_t *substr_ids, size_t n,
                            uint8_t *is_start, uint8_t *is_end);
/* match_substrs(&self, ctx, characters) integer columns for one string (lib.rs:311-773); any pointer may be NULL.
 * enable/character/masked_char/masked_substr_id: [M]; state/substr_id/start_enable/end_enable: [D][M]. */
int hrx_match_substrs(hrx_ctx *ctx, const uint8_t *characters, size_t n, size_t M, uint64_t *enable,
                      uint64_t *character, uint64_t *state, uint64_t *substr_id, uint64_t *start_enable,
                      uint64_t *end_enable, uint64_t *masked_char, uint64_t *masked_substr_id,
                      uint64_t *status);

/* ------------------------------------------------------------------ */
/* Definition generation: regex -> minimal DFA (host only, no GPU)     */
/* ------------------------------------------------------------------ */

/* The table step in front of the witness path, without V8: what DecomposedRegexConfig::gen_regex_files
 * (src/vrm/mod.rs:62-95) obtains from get_dfa_json_value -> regexToDfa (src/vrm/js_caller.rs:43-48,
 * src/vrm/regex.js:40-92) and dfa_to_regex_def_text (src/vrm/js_caller.rs:127-157).  `regex` is the concatenation of
 * the parts' regex_def, UTF-8, in the dialect of regex.js:236-367.  Byte-identical to the reference's output
 * (state numbering included).  Two-call pattern: *needed receives the byte length of the result; min(needed, cap)
 * bytes are written to out (no terminator); out may be NULL with cap 0.  A malformed pattern returns HRX_ERR_PARSE
 * with the parser's message ("Error: empty input at 2." ...) in hrx_last_error(). */
int hrx_regex_to_allstr_text(const char *regex, size_t regex_len, char *out, size_t cap, size_t *needed);
/* The intermediate value itself: the JSON text regexToDfa returns ([{"type":..,"edges":{key:target}}, ...]). */
int hrx_regex_to_dfa_json(const char *regex, size_t regex_len, char *out, size_t cap, size_t *needed);

/* DecomposedRegexConfig::gen_regex_files (src/vrm/mod.rs:62-307) as a whole: the AllstrRegexDef text of the
 * concatenated parts and one SubstrRegexDef text per public part (extract_substr_ids, mod.rs:309-538;
 * get_substr_defs_from_path, mod.rs:540-600; text format mod.rs:268-304).  The part regexes are searched in the
 * DFA's paths with leftmost-first semantics (what fancy-regex 0.11 / the regex crate do for these patterns);
 * pattern syntax outside the subset formatRegexPrintable emits from the DFA dialect -> HRX_ERR_PARSE. */
typedef struct hrx_regex_part {
    const char *regex_def; /* UTF-8, not terminated */
    size_t regex_len;
    int is_public;
    size_t max_size;
} hrx_regex_part;
typedef struct hrx_regex_files hrx_regex_files;
int hrx_gen_regex_files(const hrx_regex_part *parts, size_t n_parts, size_t max_byte_size, hrx_regex_files **out);
size_t hrx_regex_files_num_substrs(const hrx_regex_files *files);
/* pointers stay valid until hrx_regex_files_destroy; texts are not terminated, *len receives the byte length */
const char *hrx_regex_files_allstr(const hrx_regex_files *files, size_t *len);
const char *hrx_regex_files_substr(const hrx_regex_files *files, size_t idx, size_t *len);
void hrx_regex_files_destroy(hrx_regex_files *files);
/* format_regex_str (src/vrm/js_caller.rs:36-41 -> formatRegexPrintable, src/vrm/regex.js:24-39); two-call pattern */
int hrx_format_regex_str(const char *regex, size_t regex_len, char *out, size_t cap, size_t *needed);
/* The search gen_regex_files runs per part and path: leftmost-first match of `pattern` in `text`.
 * *found = 0/1; [*start, *end) the match. */
int hrx_regex_find(const char *pattern, size_t pattern_len, const char *text, size_t text_len, int *found, size_t *start,
                   size_t *end);

#ifdef __cplusplus
}
#endif
#endif /* HRX_H */
