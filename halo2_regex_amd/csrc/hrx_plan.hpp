// hrx_plan.hpp — the launch planner (hrx_plan.cpp): pure host functions from a config and a shape to the kernel, its geometry and, for a whole
// witness call, the ROUTE of launches.  hrx_api.cpp executes what they return, hrx_describe_api.cpp prints it: neither decides anything itself.
#pragma once
#include <string>
#include <vector>

#include "hrx_kernel.hpp"

namespace hrx {

// ---- one launch.  The planners read their arguments and return everything they decide in LaunchInfo; apply_plan copies the part of it that
// the kernels read out of WitnessArgs (gs, n_groups, sm_no_touch, sm_bufs) into the launch arguments.
// Picks the launch geometry for `a` on a device with `num_cus` CUs; returns false if nothing fits.
bool plan_witness_launch(const WitnessArgs &a, int num_cus, LaunchInfo &out);
// a whole config of 4 .. 8 defs in one def-parallel launch on the CLASS-WIDE tables (a.cw_image set): position-major outputs ...
bool plan_pmd_cw(const WitnessArgs &a, int num_cus, LaunchInfo &out);
// ... and string-major outputs straight out of the launch (four and five defs, rows in multiples of 16)
bool plan_pmd_cw_sm(const WitnessArgs &a, int num_cus, LaunchInfo &out);
void apply_plan(WitnessArgs &a, const LaunchInfo &li);
uint32_t plan_nt_mix(const WitnessArgs &a, const LaunchInfo &li);
// fused for D <= 3 on the narrow table in LDS where it fits, else the HALF table, else the narrow table out of L2 (the forced BYTE / HALF / global-table
// bits pick among these); via rows for more defs, where the witness planner walks in chunks (few long strings), or when forced (kDbgMatchViaRows)
bool plan_match_launch(const WitnessArgs &a, int num_cus, bool via_rows, MatchPlan &out);
// HRX_OPT_MATCH_FUSED_WIDE: does the fused walk on the CLASS-WIDE image (hrx_kernel_match_wide.hip) serve this config and shape?  True (out.wide = the defs a sweep
// walks side by side) iff the option is on, the set has 4 .. kMaxDefsPerLaunch defs and a CLASS-WIDE image that fits LDS,
// via_rows (kDbgMatchViaRows) is not set, no launch of the via-rows witness route of this shape is chunked and the input is not position-major.  False: `out`
// untouched, plan_match_launch decides as before.  layout: HRX_LAYOUT_STRING_MAJOR (ragged and selected calls too) or HRX_LAYOUT_INPUT_POSITION_MAJOR
bool plan_match_wide(const DefsSet &s, uint32_t debug, bool via_rows, bool option, int layout, size_t B, size_t M, int num_cus, MatchPlan &out);

// ---- the table fields of a launch's arguments: the ONE place a WitnessArgs is filled from a DefsSet.  The launch passes the set's device images,
// the planning-only callers the host images (host_images): the planner only looks at which images exist and how large they are.
struct SetImages {
    const uint32_t *table = nullptr;
    const uint64_t *wide = nullptr;
    const uint16_t *half = nullptr;
    const uint8_t *pair = nullptr, *byte = nullptr;
    const uint8_t *cw = nullptr;      // the CLASS-WIDE image: the arguments are those of the def-parallel kernel on it (cw_consts; table_bytes = its size)
};
SetImages host_images(const DefsSet &s, bool class_wide = false);
WitnessArgs witness_args_of(const DefsSet &s, const SetImages &im);

// ---- the route of a witness call (launch_batch): which launches serve a config, layout and shape, each with its plan.
struct BatchRoute {
    enum class Case {
        OneLaunch,          // up to kMaxDefsPerPass defs: one launch (passes[0])
        ClassWide,          // 4 .. 8 defs on the CLASS-WIDE tables: one def-parallel launch, position-major outputs
        ClassWideSm,        // ... four and five defs, string-major rows in multiples of 16: the launch writes the caller's rows itself
        ClassWideGroups,    // more than eight defs: a def-parallel pass per CW group of 4 .. 8 defs, then the summary combine
        GroupsOfThree,      // passes over groups of kMaxDefsPerPass defs; merge_last / summary_mode say how they end
    } kind = Case::OneLaunch;
    bool transpose = false;     // the launches write position-major rows into context scratch, transpose_pm_to_sm_kernel turns them around
    int layout = 0;             // the layout every inner launch runs in
    bool summary_mode = false;  // GroupsOfThree: the passes write the caller's record planes and tile summaries (else private records: copy-mode combine)
    bool merge_last = false;    // GroupsOfThree: the last pass merges the earlier summaries itself, witness_merge_status_kernel ends the call
    struct Pass {
        const DefsSet *set;     // the config, or the group of it that this launch walks
        uint32_t first_def;     // of the config
        int layout;             // the layout this launch runs in (the route's, but for the private records of a copy-mode pass: position-major)
        uint32_t debug;         // the launch's debug bits: the caller's, plus what the route forces (a summary pass is the loader / walker / finisher kernel, ...)
        uint32_t rec_stripes;   // 2: one def's record plane in two row stripes
        LaunchInfo li;
    };
    std::vector<Pass> passes;
};
// rec_pitch: rows between strings of string-major records (0: M).  n_planes: record planes the caller passes (0: none); strict_planes: refuse
// configs that cannot take planes as launch_batch does (the describe functions print such a config's launches without the planes).
// Returns HRX_OK, or an HRX_ERR_* code with its message in err.
int plan_batch_route(const DefsSet &s, uint32_t debug, uint32_t tune, bool mp_combine, int layout, size_t B, size_t M, size_t rec_pitch, int num_cus,
                     size_t n_planes, bool strict_planes, BatchRoute &out, std::string &err);

// ---- the chunked verify's chunk (hrx_ctx_verify_chunk_rows): a multiple of 64 rows; >= M: one chunk
constexpr size_t kVerifyChunkFloor = 256;
size_t plan_verify_chunk_rows(size_t B, size_t M, int num_cus);

}  // namespace hrx
