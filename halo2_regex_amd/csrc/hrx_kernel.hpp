// hrx_kernel.hpp — host-visible launch interface of the HIP kernels (hrx_kernel.hip: dispatch, auxiliary kernels; hrx_kernel_pm.hip / hrx_kernel_sm.hip: the witness kernels;
// the planner that fills LaunchInfo: hrx_plan.hpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "hrx_defs.hpp"
#include "hrx_extract.hpp"
#include "hrx_route.hpp"
#include "hrx_rows.hpp"

namespace hrx {

struct LaunchInfo;
struct WitnessArgs;
constexpr uint32_t kMaxDefsPerLaunch = 8;   // RegexDefs per config: the status word carries 8 accept bits (include/hrx.h)

struct WitnessArgs {
    const uint8_t *chars;
    uint64_t stride;
    const uint32_t *lens;
    uint32_t B, M;
    uint32_t rec_pitch, msk_pitch;  // rows between consecutive strings in records / masked (>= M), string-major layout
    uint32_t layout;                // 0 string-major [B][pitch][D] / [B][pitch]; 1 position-major [M/4][D][B][4] / [M/8][B][8]
    uint32_t *records;
    uint16_t *masked;
    uint64_t *status;
    const uint32_t *table_image;  // device copy of DefsSet::table_image
    uint32_t table_bytes;
    const uint64_t *wide_image;   // device copy of DefsSet::wide_image (same byte size as table_image), or NULL
    const uint16_t *half_image;   // device copy of DefsSet::half_image (the exact LDS image, half_bytes long), or NULL
    uint32_t half_bytes;
    const uint8_t *byte_image;    // device copy of DefsSet::byte.image (the exact LDS image: next-state bytes, disp, pair slots), or NULL
    uint32_t byte_bytes, byte_ptab_off, byte_mul_a4, byte_mul_b4, byte_slot_mask4, byte_dead;   // (mul_a * 4, mul_b * 4, (slots - 1) * 4: byte offsets of the 4-byte pair slots)
    uint32_t byte_one_id;         // BYTE table, position-major: the def's ONE substring id (0: it has several, or none): the finisher then holds three tiles instead of two (hrx_kernel_pm.hip)
    uint32_t byte_rows_bytes, byte16_bytes, byte16_ptab_off;   // the walker/storer kernel's image: next-state bytes [0, byte_rows_bytes) + the 2-byte slots (byte_image + byte_bytes) at byte16_ptab_off
    const uint8_t *cw_image;      // device copy of DefsSet::cw_image (CLASS-WIDE tables of a whole config of 4 .. 8 defs: hrx_kernel_pmd.hip CW; table_bytes = its size then), or NULL
    uint32_t cw_lut_off;          // LDS offset of def 0's class LUT
    const uint8_t *pair_image;    // device copy of DefsSet::pair.image (the exact LDS image: blocks + class LUT), or NULL
    uint32_t pair_bytes, pair_classes, pair_blk_bytes, pair_lut_off;
    uint32_t n_groups;            // ceil(B / gs): the planner's LaunchInfo::n_groups (apply_plan)
    uint32_t gs;                  // strings per wave (64, 32 or 16): LaunchInfo::gs (apply_plan)
    uint32_t D;
    uint32_t debug;               // the context's kDbg* bits below (forced kernel / table choices for the tests; ablations only with -DHRX_ABLATION)
    uint32_t tune;                // the context's kTune* bits (hrx_ctx_set_option, include/hrx.h): choices between variants that compute the same rows
    unsigned long long *stamps;   // profiling only (tools/kbench): per wave and tile 4 s_memtime stamps; NULL in the product
    // dynamic group assignment (position-major kernel, batches of >= 8 long groups per walker pair): after its first group a pair
    // takes the next unclaimed group from a device counter (hrx_kernel_pm.hip); 0 / NULL: groups g_first + j * stride
    uint32_t *group_counter;
    uint32_t group_base, group_first_dyn;
    // one pass of a multi-pass config (more than kMaxDefsPerPass defs; position-major outputs): this launch walks defs
    // rec_d0 .. rec_d0 + D - 1 of a config of rec_D defs and writes their record planes straight into the caller's buffer
    // ([M/4][rec_D][nb][4]); instead of (meaningless per-group) masked rows its finisher writes the tile summaries the combine
    // kernel needs — per tile and string 80 bytes: ST / EN bitvectors + one substr-id byte per row, [tile][5][B][16 B]
    uint32_t rec_D, rec_d0;       // 0 / 0: this launch's defs are the whole config
    uint32_t *summary;            // NULL: an ordinary launch
    // RECORD PLANES (include/hrx.h hrx_witness_batch_device_planes): def d's records in a buffer of its own — per block of kPmBlock strings [ceil(M/4)][nb][4], the
    // D = 1 position-major layout — instead of plane d of the interleaved [M/4][D][nb][4].  A D = 3 launch writes 12 of its 14 output bytes per row into the records;
    // as ONE allocation they lie in one class of the physical address space and the launch runs at what one class absorbs (the no-compute pass of cfg 4:
    // 0.70-0.77 of peak), as separately placed planes at 0.86 (profiles/r06_probes/plane_probe.txt).  rec_planes[0] == NULL: the interleaved layout, `records`.
    unsigned char *rec_planes[kMaxDefsPerLaunch];
    // ... and ONE def's plane in two ROW STRIPES (rec_stripes == 2, D == 1): quad q of a string in buffer q % 2 at slot q / 2 — per block [ceil(ceil(M/4)/2)][nb][4] each — so that even a
    // one-def launch's 4 record bytes per row spread over two classes of the address space beside the masked rows' third (the no-compute pass of the bench line 0.76 -> 0.805 of peak,
    // of cfg 5's byte count 0.72-0.80 -> 0.82: profiles/r06_probes/stripe_probe_*.txt).  0 / 1: whole planes.
    uint32_t rec_stripes;
    // the LAST pass of a multi-pass config reads the earlier groups' tile summaries itself (its finisher has everything else in hand: this
    // group's bitvectors and id bytes, the input bytes, the reveal-mask carries) and writes the FINAL masked rows: no combine launch,
    // this group's summary never written, the others' read once.  0: not such a pass.
    uint32_t merge_G;                              // earlier groups (<= kMaxMergeGroups)
    const uint32_t *merge_summary[3];              // their WitnessArgs::summary buffers
    uint32_t *merge_ov;                            // [B]: lowest row that defs of DIFFERENT groups flag together (0xffffffff: none) -> witness_merge_status_kernel
    // chunked launch of the loader / walker / finisher kernel (hrx_kernel_spec.hip): NULL / 0 in an ordinary launch
    const uint32_t *vs_init;      // [chunk][B][D]: state | substr id of the transition into the chunk's first row << 16 | its end flag << 24
    uint32_t vs_chunks, vs_tiles, vs_groups;   // chunks per string, tiles per chunk, REAL groups (n_groups = vs_groups * vs_chunks)
    uint64_t *vs_status;          // [chunk][B]: every chunk's status word
    uint2 *vs_info;               // [chunk][B]: pend | fwd << 1 | sm << 2 | dec << 3, pend_start (hrx_lane.h TileMasks)
    uint32_t sm_no_touch;         // walker/storer kernel: 1 = the storer does not warm L2 for the walker (LaunchInfo::sm_no_touch, apply_plan; hrx_kernel_sm.hip)
    uint32_t sm_bufs;             // def-parallel kernel, string-major outputs: LDS sub-tile buffers per group, 2 or 3 (LaunchInfo::sm_bufs, apply_plan; hrx_kernel_pmd.hip SMO)
    uint32_t nt_mix;              // position-major kernels: which stores are write-back instead of streaming (kNtMix*, hrx_kernel_pm.hip)
    uint32_t pace_even;           // profiling only (HRX_PACE, stamps / ablation builds): x 64 idle cycles per tile for the walkers of even workgroups; 0 in the product
    DefConsts dc[kMaxDefsPerLaunch];
};

// HRX_DEBUG_FLAGS (environment; read ONCE per context in hrx_ctx_create, never per launch).  The "force" bits let the
// parity tests drive every kernel / table format through the same batches; they change which kernel runs, never what it
// computes.  The ablation bits (stores skipped, input re-read from L2, ...) make the OUTPUT WRONG: they exist only in a
// library built with -DHRX_ABLATION (`make ablation` -> libhrx_ablation.so, used by tools/ only); in the release
// libhrx.so their enumerators are 0, so every `a.debug & kDbgSkip...` test folds to false at compile time and no
// environment variable can make a launch skip work.
#ifdef HRX_ABLATION
#define HRX_ABL(x) (x)
#else
#define HRX_ABL(x) 0u
#endif
enum : uint32_t {
    kDbgSkipRecords = HRX_ABL(1u),             // ablation: no record stores
    kDbgSkipMasked = HRX_ABL(2u),              // ablation: no masked-row stores
    kDbgInputFromL2 = HRX_ABL(4u),             // ablation: every tile re-reads the first input lines (no HBM reads) / no prefetch of the next tile
    kDbgNoTouch = HRX_ABL(8u),                 // ablation, walker/storer kernel: no L2 touch-ahead of the input
    kDbgSplitNoWalk = HRX_ABL(16u),            // ablation, walker/storer kernel: storers move whatever the slots hold
    kDbgNoNtRecords = HRX_ABL(32u),            // ablation, position-major kernels: ordinary record stores
    kDbgNoNtMasked = HRX_ABL(64u),             // ablation, position-major kernels: ordinary masked-row stores
    kDbgNoNtStores = HRX_ABL(96u),             // both (the release build's stores are non-temporal at compile time: no branch per store)
    kDbgPpNoTranslate = HRX_ABL(0x100u),      // ablation, pair-step kernel: the loader skips the class lookups (pair index 0 everywhere)
    kDbgPpNoPost = HRX_ABL(0x200u),            // ablation, pair-step kernel: the walker only follows the chain (no records, flags, ids)
    kDbgPpNoMask = HRX_ABL(0x400u),            // ablation, pair-step kernel: no reveal-mask work at the tile end
    kDbgSkipFixups = HRX_ABL(0x800000u),       // ablation: no end-mask fix-ups
    kDbgFixedLines = HRX_ABL(0x1000000u),      // ablation: every quad / octet of a string is stored onto its first one
    kDbgFixToDummy = HRX_ABL(0x4000u),         // ablation: the end-mask repairs are stored onto the string's first octets (same instructions, no read-modify-write at the memory)
    kDbgForceOneWave = 0x10000u,      // string-major: the one-wave kernel instead of the walker/storer kernel
    kDbgGroups32 = 0x20000u,          // one-wave kernel: 32 strings per wave
    kDbgForceGlobalTable = 0x40000u,  // walk the fused table out of global memory even if it fits LDS
    kDbgForceNarrow = 0x80000u,       // position-major kernel: 4-byte table even where the planner picks WIDE
    kDbgForceWide = 0x200000u,        // position-major kernel: WIDE table also at D = 1
    kDbgForceHalf = 0x400000u,        // position-major kernel: HALF table even if the 4-byte one fits LDS
    kDbgForceByte = 0x2000u,          // position-major kernel, one def: BYTE table even if the 4-byte one fits LDS
    kDbgNoByte = 0x8000u,             // position-major kernel: never the BYTE table (the HALF table where the 4-byte one does not fit)
    kDbgNoDefParallel = 0x2000000u,   // position-major: never the def-parallel kernel
    kDbgForceDefParallel = 0x4000000u,// position-major, D >= 2, WIDE table: the def-parallel kernel whatever the batch size (tests)
    kDbgNoPair = 0x8000000u,          // position-major, D = 1: never the pair-step kernel (hrx_kernel_pp.hip)
    kDbgForcePair = 0x40000000u,      // position-major, D = 1 with a PAIR table: the pair-step kernel whatever the batch size (tests, A/B)
    kDbgNoDynamicGroups = 0x1u << 11,  // position-major kernel: static group assignment whatever the batch size
    kDbgForceDynamicGroups = 0x1u << 12,   // ... dynamic from two groups per walker and any row count (tests)
    kDbgXcdRemap = 0x100000u,         // position-major kernels: every XCD walks a CONTIGUOUS eighth of the groups (hrx_device.h xcd_slot; measured 1.5 % slower, off by default)
    kDbgForceSpec = 0x80u,            // position-major: the chunked launch (hrx_kernel_spec.hip) whatever the batch size, chunks of 4 tiles (tests)
    kDbgNoSpec = 0x80000000u,         // position-major: never the chunked launch
    kDbgForceHost = 0x10000000u,      // host-buffer entry points: always the native host walk (hrx_host_walk.cpp)
    kDbgNoHost = 0x20000000u,         // host-buffer entry points: never the native host walk
    // every bit that merely selects a kernel (the only ones a release build honours)
    kDbgForceMask = kDbgForceOneWave | kDbgGroups32 | kDbgForceGlobalTable | kDbgForceNarrow | kDbgForceWide | kDbgForceHalf | kDbgForceByte | kDbgNoByte |
                    kDbgNoDefParallel | kDbgForceDefParallel | kDbgNoPair | kDbgForcePair | kDbgXcdRemap | kDbgNoDynamicGroups | kDbgForceDynamicGroups | kDbgForceHost | kDbgNoHost |
                    kDbgForceSpec | kDbgNoSpec,
#ifdef HRX_ABLATION
    kDbgHonoured = 0xffffffffu,
#else
    kDbgHonoured = kDbgForceMask,
#endif
};
// hrx_ctx_set_option (include/hrx.h) -> WitnessArgs::tune
enum : uint32_t {
    kTunePmdFinMask = 3u, kTunePmdFinOn = 1u, kTunePmdFinOff = 2u,   // HRX_OPT_PMD_COMBINER_WAVE: the def-parallel kernel on the WIDE table with / without a combiner wave (0: the planner's default)
};
// HRX_DEBUG_FLAGS from the environment, reduced to the bits this build honours
uint32_t debug_flags_from_env();
// ... and the one bit above the 32 of WitnessArgs::debug: the match entry points (hrx_match_batch_device) go "via rows" whatever the planner says (tests)
constexpr uint64_t kDbgMatchViaRows = 1ull << 32;
bool match_via_rows_from_env();

enum class Kernel {
    OneWave,   // one-wave-does-all kernel (witness_kernel)
    Split,     // walker/storer kernel (witness_split_kernel)
    Pm,        // loader/walker kernel for the position-major layout (witness_pm_kernel)
    Pmd,       // def-parallel loader/walker kernel for D >= 2 batches that leave walker slots empty, or a whole config on the CLASS-WIDE tables (witness_pmd_kernel)
    Pp,        // pair-step loader/walker kernel, position-major, D = 1 (witness_pp_kernel: two bytes per dependent lookup)
};
struct LaunchInfo {
    Kernel kernel;
    int waves_per_wg;  // split: 2 * pairs
    int nslots;        // split: ring slots per walker/storer pair
    int gtab;          // 1: fused table read from global memory (too large for LDS)
    int wide;          // 1: position-major kernel on the WIDE table (hrx_lane.h)
    int half;          // 1: position-major kernel on the HALF table (hrx_lane.h)
    int byte;          // 1: position-major kernel on the BYTE table (hrx_lane.h): walker + loader + finisher
    int grid;
    int dyn;           // 1: dynamic group assignment (position-major loader/walker kernel, >= 8 long groups per walker pair)
    int spec_tiles;    // > 0: CHUNKED launch (hrx_kernel_spec.hip): tiles per chunk; the geometry above is that of the walk over the chunks
    int spec_chunks;   // chunks per string
    int pmd_fin;       // def-parallel kernel on the WIDE table (two and three defs): 1 = a combiner wave of its own per group (hrx_kernel_pmd.hip FIN)
    size_t lds_bytes;
    // what the kernels read out of WitnessArgs of the planner's choices (apply_plan copies them there)
    uint32_t gs;           // strings per wave: 64; the one-wave kernel: 64, 32 or 16
    uint32_t n_groups;     // ceil(B / gs); a chunked launch: the REAL groups (its walk runs over n_groups x spec_chunks)
    uint32_t sm_no_touch;  // walker/storer kernel: 1 = the storer does not warm L2 for the walker
    uint32_t sm_bufs;      // def-parallel kernel, string-major outputs: LDS sub-tile buffers per group, 2 or 3
};

// LDS bytes one wave stages per 64-string x 64-row tile
constexpr size_t wave_stage_bytes(int D, unsigned gs) { return ((size_t)gs + 1) * ((256 * (size_t)D + 16) + 80 + 8); }
constexpr size_t kLdsLimit = 160 * 1024;

hipError_t launch_witness(const WitnessArgs &a, const LaunchInfo &li, hipStream_t stream);
hipError_t launch_zero_u32(uint32_t *p, hipStream_t stream);   // *p = 0 as a kernel node (hrx_kernel.hip)
// the kernel translation units behind launch_witness: Kernel::Pm -> hrx_kernel_pm.hip, OneWave and Split -> hrx_kernel_sm.hip,
hipError_t launch_witness_pm(const WitnessArgs &a, const LaunchInfo &li, hipStream_t stream);
hipError_t launch_witness_sm(const WitnessArgs &a, const LaunchInfo &li, hipStream_t stream);
hipError_t launch_witness_pmd(const WitnessArgs &a, const LaunchInfo &li, hipStream_t stream);   // Pmd -> hrx_kernel_pmd.hip
hipError_t launch_witness_pp(const WitnessArgs &a, const LaunchInfo &li, hipStream_t stream);    // Pp -> hrx_kernel_pp.hip
// position-major loader/walker kernel (hrx_kernel_pm.hip): LDS bytes per walker/loader pair.  FIN = the loader also finishes
// the tiles (reveal masks + masked rows) from a 6-KiB summary the walker hands over; not for the HALF table (a 256-state table
// leaves no LDS for it) nor for string-major outputs.
// nt_mix: low byte k: the records of every k-th tile (t % k == k - 1) are stored write-back, 0 = all streaming; bit 8: the masked
// rows write-back.  plan_nt_mix (hrx_plan.cpp) picks k so that ~128 MiB of a launch's records stay write-back.  Whatever it says, the
// masked rows of a tile into which an OPEN optimistic span reaches are written back: they may be zeroed later, and a repair that finds
// its line in L2 costs the memory nothing (hrx_kernel_pm.hip octets_out).  Tools only (the libhrx_ntenv.so build reads HRX_NT_MIX /
// HRX_NT_FLAGS at every launch, tools/ab_policy.py): bit 9 = not even those, bits 12-15 km = the masked rows of every km-th tile as well.
constexpr uint32_t kNtMixMaskedWb = 0x100u, kNtMixNoOpenSpan = 0x200u;
// hrx_place.hip: microseconds (device clock) of a time-aligned two-stream write over two regions (both are overwritten); clk: 16 bytes of device scratch
double placement_probe_us(void *rec, size_t rec_bytes, void *msk, size_t msk_bytes, uint32_t D, hipStream_t st, unsigned long long *clk, size_t *bytes_written);
// hrx_place.hip: the memory traffic of one position-major witness launch of this shape and nothing else (roofline diagnostics)
hipError_t launch_traffic_pass_sm(const uint8_t *chars, size_t stride, size_t B, size_t M, uint32_t D, uint32_t *records, size_t rec_pitch, uint16_t *masked,
                                  size_t msk_pitch, uint32_t nt_mix, uint32_t *sink, int num_cus, hipStream_t stream);
hipError_t launch_traffic_pass(const uint8_t *chars, size_t stride, size_t B, size_t M, uint32_t D, uint32_t *records, uint16_t *masked,
                               uint32_t nt_mix, uint32_t *sink, int num_cus, hipStream_t stream, uint32_t *const *planes = nullptr, uint32_t stripes = 1);
constexpr size_t kPmSummaryBytes = 6144;
template <bool HALF, bool SM> constexpr bool kPmFinisher = !HALF && !SM;
constexpr int pm_max_threads(bool half, bool sm) { return (!half && !sm) ? 768 : 512; }
constexpr size_t kPmCounterBytes = 128;   // ready / freed / freed2 / sum_ready / sum_freed / gq_ready + the 16-entry group queue
constexpr size_t pm_pair_bytes(size_t nring, bool half, bool fin) { return nring * 4096 + (half ? 0 : 4096) + (fin ? kPmSummaryBytes : 0) + kPmCounterBytes; }
constexpr size_t kPpSlotBytes = 8192;   // pair-step kernel: one ring slot = 4 KiB of pair indices + 4 KiB of raw bytes
constexpr size_t pp_pair_bytes(size_t nring) { return nring * kPpSlotBytes + kPmSummaryBytes + kPmCounterBytes; }   // + the finisher's tile summary + counters
// LDS bytes per group of the def-parallel kernel: input ring + (D - 1) x (2 summaries of 5 KiB + a 2-KiB status piece) + counters
constexpr size_t pmd_group_bytes(int D, int nring) { return (size_t)nring * 4096 + (size_t)(D - 1) * (2 * 5120 + 2048) + 192; }
// ... of the WIDE kernel with a combiner wave (FIN): all D walkers publish, their status pieces lie in their first summary slots (hrx_kernel_pmd.hip PA)
constexpr size_t pmd_fin_group_bytes(int D, int nring) { return (size_t)nring * 4096 + (size_t)D * (2 * 5120) + 192; }

// Configs of more than kMaxDefsPerPass RegexDefs (hrx_defs.hpp): every group of defs is walked by an ordinary launch into a
// group-private position-major records buffer [ceil(M/4)][D_g][nb][4] (blocked like every position-major buffer) and its own
// status array; witness_combine_kernel (hrx_kernel_mp.hip) then reads the groups' rows once, writes them into the caller's
// records buffer in its layout, and computes what needs ALL defs of a row: Sum(substr_id), Sum(is_start), Sum(is_end) ->
// reveal masks and masked rows (lib.rs:467-519, 593-764), the flag-overlap row, the merged status word.
constexpr uint32_t kMaxGroups = 32;
constexpr uint32_t kMaxMergeGroups = 3;   // earlier groups the last pass of a multi-pass config can merge itself (WitnessArgs::merge_summary); more: the combine launch
struct CombineArgs {
    const uint8_t *chars;
    uint64_t stride;
    const uint32_t *lens;
    uint32_t B, M, D, G;
    uint32_t layout;                // the CALLER's layout: bit 0 position-major outputs, bit 1 position-major input
    uint32_t rec_pitch, msk_pitch;  // string-major outputs
    uint32_t *records;
    uint16_t *masked;
    uint64_t *status;
    const uint32_t *grec[kMaxGroups];      // copy mode: the groups' private records buffers; summary mode: NULL
    const uint32_t *gsummary[kMaxGroups];  // summary mode (position-major outputs): the groups' tile summaries (WitnessArgs::summary)
    const uint32_t *merge_ov;              // launch_merge_status: WitnessArgs::merge_ov of the last pass
    const uint64_t *gstatus[kMaxGroups];
    uint8_t gD[kMaxGroups], gfirst[kMaxGroups];
};
hipError_t launch_combine(const CombineArgs &a, hipStream_t stream);
// the status words of a multi-pass config whose last pass merged the summaries itself: one thread per string (bad length, the lowest def's
// undefined transition, the lowest overlap row, the accept bits of all groups)
hipError_t launch_merge_status(const CombineArgs &a, hipStream_t stream);

// CHUNKED walk (hrx_kernel_spec.hip): scout -> compose -> the loader / walker / finisher kernel over chunks (WitnessArgs::vs_*) -> stitch
constexpr uint32_t kSpecMaxChunks = 32, kSpecMaxChunkTiles = 64;
struct SpecArgs {
    const uint8_t *chars;
    uint64_t stride;
    const uint32_t *lens;
    uint32_t B, M, D;
    uint32_t in_pm;                          // 1: position-major input ([stride/16][B][16]), 0: string-major ([B][stride])
    uint32_t C, tiles_per_chunk, n_groups;   // chunks per string, 64-row tiles per chunk, REAL groups of 64 strings
    const uint32_t *table_image;             // the narrow fused table (global copy; the scout stages it into LDS)
    uint32_t table_bytes;
    DefConsts dc[kMaxDefsPerLaunch];
    uint32_t n_states[kMaxDefsPerLaunch];    // real states per def (largest + 1)
    uint32_t qabs[kMaxDefsPerPass][8];       // bit s: real state s is quasi-absorbing — every byte keeps it where it is, except bytes that NO real state
                                             // of the def has a transition for (those send it to the dead row, like everybody else)
    uint32_t smax;                           // >= every n_states
    // COMPACT scout tables (hrx_api.cpp build_scout_image): per def a 256-byte class LUT (byte -> 2 x its column class) and the transition table over
    // CLASSES, u16 entries holding the LDS byte address of the next state's row: a row is a few dozen bytes, so the lanes of a wave — different strings, mostly the
    // same few states — read a handful of dwords instead of 64 random ones (the 4-byte [state][byte] table costs ~4.5 bank-conflict passes per wave read).
    // cimage == NULL: some def has more than 127 classes (or the image passes 64 KiB): the scout walks the narrow table.
    const uint8_t *cimage;
    uint32_t cimage_bytes;
    uint32_t c_lut[kMaxDefsPerPass], c_tab[kMaxDefsPerPass], c_rowb[kMaxDefsPerPass], c_inv[kMaxDefsPerPass];   // LDS offsets of LUT and table, bytes per row, ceil(2^16 / rowb)
    const uint16_t *pair_tags[kMaxDefsPerLaunch];   // device (state, next) -> tag tables (hrx_defs.hpp pair_tags)
    // scratch: one row per (chunk, def, string), [chunk][def][n_groups * 64][row_bytes]: smax bytes "the state start state s reached after
    // the scout's stage A" + a 32-byte record (8 keys | where each key ends | where it is before the chunk's last byte | fail flag)
    uint8_t *rows;
    uint32_t row_bytes;                      // smax + 32, a multiple of 16
    uint32_t dbg;                            // profiling only (ablation build, HRX_SPEC_DBG): 1 no tag load, 2 no init store in compose
    uint32_t *init;                          // [chunk][B][D] -> WitnessArgs::vs_init
    const uint2 *vinfo;                      // [chunk][B] <- WitnessArgs::vs_info
    const uint64_t *vstatus;                 // [chunk][B] <- WitnessArgs::vs_status
    uint64_t *status;
    const uint32_t *records;
    const uint32_t *rec_planes[kMaxDefsPerPass];   // record planes (WitnessArgs::rec_planes): def d's records in a buffer of its own; rec_planes[0] == NULL: the interleaved `records`
    uint16_t *masked;
    // chunks whose reveal-mask assumptions were wrong, found by the stitch launch, recomputed by the repair launch (one wave each)
    uint32_t *work_count;                    // [1], zeroed in front of the stitch launch
    uint2 *work;                             // [work_cap]: string, chunk | true start_mask before it << 8 | true end_mask of its last row << 9
    uint32_t work_cap;
};
hipError_t launch_spec_scout(const SpecArgs &a, int num_cus, hipStream_t stream);
hipError_t launch_spec_compose(const SpecArgs &a, hipStream_t stream);
hipError_t launch_spec_stitch(const SpecArgs &a, int num_cus, hipStream_t stream);

// MATCH (include/hrx.h hrx_match_batch_device; hrx_kernel_match.hip): status + revealed runs, no witness rows.
//   fused:     match_lane_kernel<D, GTAB, HALF> — one lane per string on the narrow fused table (in LDS, or out of L2: GTAB) or the HALF table
//              (in LDS), the lane algorithm of hrx_host_walk.cpp with no row stores, tile_masks + SpanEmitter (hrx_lane.h) at every tile end.
//              The per-string state, the tile step and the status epilogue are the lane core of hrx_match_tile.h (MatchLane), which the ragged
//              kernel below shares; so is the launch ladder over D and the table form (fused_kernel)
//   via rows:  the position-major witness launch into context scratch, then spans_from_masked_pm_kernel over its masked rows
constexpr uint32_t kMatchThreads = 256;     // most lanes (strings) per workgroup of the fused kernel
constexpr uint32_t kMatchMaxSpans = 1u << 16;
constexpr size_t kMatchScratchBytes = (size_t)768 << 20;    // "via rows" witness slices (DevBuf rounds it up by a quarter: < 1 GiB)
struct MatchArgs {
    const uint8_t *chars;
    uint64_t stride;
    const uint32_t *lens;
    uint32_t B, M, D;
    uint32_t in_pm;                 // 1: input [stride/16][nb][16] per block of kPmBlock strings
    const uint32_t *table_image;    // the narrow fused table (device copy): staged into LDS, or read in place (GTAB)
    const uint16_t *half_image;     // the HALF table (device copy), staged into LDS
    uint32_t table_bytes;           // bytes staged into LDS (0: GTAB)
    const uint16_t *masked;         // spans_from_masked_pm_kernel: the slice's position-major masked rows [ceil(M/8)][nb][8], blocked
    uint64_t *status;
    uint32_t *span_counts;          // may be NULL
    uint64_t *spans;                // [B][max_spans], NULL when max_spans == 0
    uint32_t max_spans;
    DefConsts dc[3];
};
struct MatchPlan {
    int fused;          // 1: match_lane_kernel<D, gtab, half>; 0: via rows
    int wide;           // > 0: the fused walk for four to eight defs instead, match_wide_kernel<D, wide, Src, SEL> on the CLASS-WIDE image (plan_match_wide)
    int gtab, half;
    int grid, threads;
    size_t lds_bytes;
};
hipError_t launch_match_lane(const MatchArgs &a, const MatchPlan &p, hipStream_t stream);
hipError_t launch_spans_from_masked(const MatchArgs &a, hipStream_t stream);
// position-major input of strings [b0, b0 + n) (all in one block of kPmBlock) -> string-major [n][stride] (the "via rows" slices inside a block)
hipError_t launch_pm_input_slice(const uint8_t *chars_pm, size_t stride, size_t B, size_t b0, size_t n, uint8_t *out, hipStream_t stream);

// RAGGED input (include/hrx.h hrx_match_batch_device_ragged, hrx_ragged_to_position_major_device; hrx_kernel_ragged.hip): string b is the bytes
// values + (offsets[b] - base) .. values + (offsets[b + 1] - base), read as the aligned 16-byte chunks that hold them.
//   match_ragged_kernel<D, GTAB, HALF> — the fused match (plan_match_launch picks D and the table as for the padded kernel), persistent lanes:
//   the ragged addressing, window carry and realign around the same lane core
struct RaggedMatchArgs {
    MatchArgs m;                    // chars = values; stride, lens and in_pm unused
    const uint64_t *offsets;        // [B + 1]
    uint64_t base;                  // subtracted from every offset (0 on the device entry: offsets index values)
};
hipError_t launch_match_ragged(const RaggedMatchArgs &r, const MatchPlan &p, int num_cus, hipStream_t stream);
// strings [b0, b0 + n) -> string-major [n][stride] zero-padded, lens [n] (UINT32_MAX: decreasing offsets or longer than limit; no byte read)
hipError_t launch_ragged_slice(const uint8_t *values, const uint64_t *offsets, uint64_t base, size_t b0, size_t n, uint32_t limit, size_t stride,
                               uint8_t *out, uint32_t *lens, hipStream_t stream);
// the batch -> HRX_LAYOUT_INPUT_POSITION_MAJOR [stride/16][nb][16] per block, zero-padded, lens [B] (UINT32_MAX: as above, limit = stride)
hipError_t launch_ragged_to_position_major(const uint8_t *values, const uint64_t *offsets, uint64_t base, size_t B, size_t stride, uint8_t *chars_pm,
                                           uint32_t *lens, hipStream_t stream);

// SELECTED match (include/hrx.h hrx_match_selected_device): the strings sel[0 .. n_sel) of a ragged (offsets) or string-major (lens,
// src_stride) batch of B, walked in that order, results at index sel[k]; an index at or past B is passed over.
//   fused:     match_selected_kernel<D, GTAB, HALF, Src> — the ragged kernel's persistent-lane walk with the string's place and the lane's next
//              string as parameters (a kernel of its own: match_ragged_kernel stays the code it was); a.chars / stride / lens / in_pm unused, a.B = B
//   via rows:  selected_slice_kernel<Src> stages slot s = string sel[k0 + s]; the witness launch writes the slots' status words into scratch;
//              spans_from_masked_selected_kernel reads slot s and writes status, count and runs at sel[k0 + s]
struct SelectedSrc {
    const uint8_t *src;
    const uint64_t *offsets;        // ragged: [B + 1]; NULL: string-major
    const uint32_t *lens;           // string-major: [B]
    uint64_t src_stride;
};
hipError_t launch_match_selected(const MatchArgs &a, const SelectedSrc &s, const uint32_t *sel, size_t n_sel, const MatchPlan &p, int num_cus,
                                 hipStream_t stream);
hipError_t launch_selected_slice(const SelectedSrc &s, size_t B, const uint32_t *sel, size_t k0, size_t n, uint32_t limit, size_t stride, uint8_t *out,
                                 uint32_t *lens, hipStream_t stream);
// where the scan of a selected via-rows slice writes: slot s of the slice (a.status, a.masked, a.B slots) -> index sel[s] < B_src of these arrays
struct SpanScatter {
    const uint32_t *sel;            // the slice's part of the selection
    uint32_t B_src;
    uint64_t *status;
    uint32_t *span_counts;          // may be NULL
    uint64_t *spans;                // [B_src][max_spans], NULL when max_spans == 0
};
hipError_t launch_spans_from_masked_selected(const MatchArgs &a, const SpanScatter &o, hipStream_t stream);
// FUSED-WIDE match (HRX_OPT_MATCH_FUSED_WIDE; hrx_kernel_match_wide.hip, lane core and arguments: hrx_match_wide.h): four to eight defs, one lane per
// string on the CLASS-WIDE image in LDS, p.wide defs side by side.  One kernel template serves the string-major, ragged (base: subtracted from every offset) and
// selected entries: sel == NULL walks strings 0 .. a.B - 1 of the source, else sel[0 .. n_sel)
struct MatchWideArgs;
hipError_t launch_match_wide(const MatchWideArgs &a, const SelectedSrc &s, uint64_t base, const uint32_t *sel, size_t n_sel, const MatchPlan &p, int num_cus,
                             hipStream_t stream);

// EXTRACT (include/hrx.h hrx_extract_spans_device; hrx_kernel_extract.hip): the runs of a match call -> run_offsets / runs / byte_offsets / values / totals.
// Count, scan, apply, gather: four launches, nothing but the caller's workspace in between (extract_workspace_bytes: 3 words per kExtractThreads strings + 4)
constexpr uint32_t kExtractThreads = 256;       // strings per workgroup of the count and apply launches; the scan launch takes this many partials per round
struct ExtractArgs {
    ExtractIn in;                   // hrx_extract.hpp: layout, input, the match call's outputs, max_spans, require_accept
    uint64_t *run_offsets;          // [B + 1]
    uint64_t *runs;                 // [runs_cap]
    uint64_t *byte_offsets;         // [runs_cap + 1]
    uint8_t *values;                // [values_cap]
    uint64_t *totals;               // [4]
    uint64_t runs_cap, values_cap;
    uint64_t *ws;                   // the caller's workspace
};
size_t extract_workspace_bytes(size_t B);
hipError_t launch_extract(const ExtractArgs &a, hipStream_t stream);

// ROUTE (include/hrx.h hrx_route_device; hrx_kernel_route.hip): a stable partition of the batch by (kept?, length bucket) -> order / bucket_offsets.
// Count, scan, apply: three launches of kExtractThreads lanes, nothing but the caller's workspace in between
// (route_workspace_bytes: kRouteBins words per kExtractThreads strings + kRouteBins)
struct RouteArgs {
    RouteIn in;                     // hrx_route.hpp: status, require_accept, lens or offsets, B, the bounds by value
    uint32_t *order;                // [B]
    uint64_t *bucket_offsets;       // [bounds.n + 2]
    uint64_t *ws;                   // the caller's workspace
};
size_t route_workspace_bytes(size_t B);
hipError_t launch_route(const RouteArgs &a, hipStream_t stream);
// GATHERED STAGING (include/hrx.h hrx_gather_to_position_major_device; hrx_kernel_ragged.hip): slot k of the position-major output = source string sel[k]
// of a ragged (offsets) or string-major (lens, src_stride) batch of B strings; lens_out[k] = UINT32_MAX and a zero slot where sel[k] >= B or the
// string does not fit (launch_ragged_to_position_major is the same kernel without sel)
hipError_t launch_gather_to_position_major(const uint8_t *src, size_t src_stride, const uint32_t *lens, const uint64_t *offsets, size_t B,
                                           const uint32_t *sel, size_t n_sel, size_t stride, uint8_t *chars_pm, uint32_t *lens_out, hipStream_t stream);

// position-major -> string-major (hrx_kernel_tp.hip): string-major callers served by the position-major path
struct TransposeArgs {
    const uint32_t *records_pm;     // [ceil(M/4)][D][nb][4], blocked by kPmBlock strings
    const uint16_t *masked_pm;      // [ceil(M/8)][nb][8]
    uint32_t B, M, D;
    uint32_t *records;              // [B][rec_pitch][D]
    uint16_t *masked;               // [B][msk_pitch]
    uint32_t rec_pitch, msk_pitch;  // rows, multiples of 8
};
hipError_t launch_transpose(const TransposeArgs &a, hipStream_t stream);
// string-major input bytes [B][stride] -> HRX_LAYOUT_INPUT_POSITION_MAJOR (blocks of kPmBlock strings, [stride/16][nb][16]); hrx_kernel_tp.hip
hipError_t launch_chars_to_position_major(const uint8_t *chars_sm, size_t stride, size_t B, uint8_t *chars_pm, hipStream_t stream);

// states-in entry points (lib.rs:825-888): tags[d*n+i] = pair_tag(states[d][i], states[d][i+1])
hipError_t launch_pair_tags(const uint64_t *states, size_t n, uint32_t D, const uint16_t *const *pair_tags,
                            const uint32_t *n_states, uint16_t *tags, hipStream_t stream);

// derive_is_start_end (lib.rs:847-888) for caller-supplied states AND substr ids:
// flags[d*n+i] bit0 = is_start[d][i], bit1 = is_end[d][i+1]
struct EndpointArgs {
    const uint64_t *states;
    const uint64_t *substr_ids;
    uint64_t n;
    uint32_t D;
    uint8_t *flags;
};
// member[d]: device membership bytes of def d; dims[3 d .. 3 d + 2] = {n_states, n_substrs, id_offset} of def d (one launch per def)
hipError_t launch_endpoint_flags(const EndpointArgs &a, const uint8_t *const *member, const uint32_t *dims, hipStream_t stream);

// compact witness rows of strings [b_begin, b_begin + b_count) -> bn256::Fr cells, [col][string][row][4]
struct FrArgs : RowsIn {   // the rows (hrx_rows.hpp), and
    uint32_t b_begin, b_count;
    uint32_t canonical;   // 1: plain integers instead of Montgomery form
    uint64_t *cells;      // first cell of string b_begin in column 0
    uint64_t col_cells;   // cells between consecutive columns (= strings of the whole request x M)
};
hipError_t launch_fr_columns(const FrArgs &a, hipStream_t stream);

// VERIFY (hrx_kernel_verify.hip): the rules of hrx_verify.hpp over the same rows; one verdict word per string
struct VerifyArgs;     // hrx_verify.hpp
hipError_t launch_verify_rows(const VerifyArgs &a, hipStream_t stream);
struct VerifyChunkArgs;
hipError_t launch_verify_chunked(const VerifyChunkArgs &ca, hipStream_t stream);      // the chunk launch, then the stitch launch
// LOOKUP COUNTS (hrx_kernel_lookup.hip): the rule of hrx_lookup.hpp over the same row forms; a histogram per string with the bins in LDS
struct LookupArgs;     // hrx_lookup.hpp
hipError_t launch_lookup_counts(const LookupArgs &a, size_t lds_bytes, hipStream_t stream);
// LOOKUP COMPRESS (hrx_kernel_compress.hip): the rule of hrx_compress.hpp — the lookup tuples of the rows / the rows of the tables folded with a challenge
struct CompressArgs;   // hrx_compress.hpp
struct CompressTableArgs;
hipError_t launch_compress_inputs(const CompressArgs &a, hipStream_t stream);
hipError_t launch_compress_table(const CompressTableArgs &a, hipStream_t stream);
// LOOKUP PERMUTE (hrx_kernel_permute.hip): the rule of hrx_permute.hpp — the permuted columns of the lookup argument out of the counts; the overflow
// words' launch (where asked for), then the columns' launch
struct PermuteArgs;    // hrx_permute.hpp
hipError_t launch_lookup_permute(const PermuteArgs &a, hipStream_t stream);
// LOOKUP PRODUCT (hrx_kernel_product.hip): the rule of hrx_product.hpp — the inverse tables by batch inversion (one launch), and the grand product Z (one
// launch, one more for the open words)
struct InvertArgs;     // hrx_product.hpp
struct ProductArgs;
hipError_t launch_lookup_invert(const InvertArgs &a, hipStream_t stream);
hipError_t launch_lookup_product(const ProductArgs &a, hipStream_t stream);
// FR NTT (hrx_kernel_ntt.hip): the rule of hrx_ntt.hpp — the twiddle table of size 2^k (one launch), and the transform (ntt_plan(k).launches launches)
struct NttArgs;        // hrx_ntt.hpp
hipError_t launch_ntt_prepare(uint32_t k, uint32_t *ws, hipStream_t stream);
hipError_t launch_ntt(const NttArgs &a, int device, hipStream_t stream);
// LOOKUP QUOTIENT (hrx_kernel_quotient.hip): the rule of hrx_quotient.hpp — the table 1 / (X^n - 1) on the coset (one launch of one workgroup), and the
// five constraints of every lookup folded into the quotient accumulator (one launch)
struct QuotientArgs;   // hrx_quotient.hpp
struct VanishArgs;
hipError_t launch_lookup_quotient(const QuotientArgs &a, hipStream_t stream);
hipError_t launch_vanishing_inverse(const VanishArgs &a, hipStream_t stream);

}  // namespace hrx
