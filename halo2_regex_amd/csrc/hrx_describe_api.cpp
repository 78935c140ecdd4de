// hrx_describe_api.cpp — hrx_describe_launch / hrx_ctx_describe_launch: the kernel and geometry the planner picks for a shape, as text, without launching
// (what rocprofv3 will list; tests/test_abi.py pins it per config).  The text is a print-out of the route plan that launch_batch executes (hrx_plan.hpp).
#include "hrx_ctx.hpp"

using namespace hrx;

// one launch of a route; class_wide: the def-parallel kernel on the CLASS-WIDE tables
static std::string launch_text(const BatchRoute::Pass &ps, bool class_wide, size_t M) {
    const LaunchInfo &li = ps.li;
    const uint32_t D = (uint32_t)ps.set->defs.size();
    const bool sm = !(ps.layout & 1);
    char name[128], line[256];
    const char *tf[2] = {"false", "true"};
    // the names rocprofv3 lists: every template argument spelled out, defaulted ones too (an exact-match join with a kernel_stats.csv works)
    switch (li.kernel) {
        case Kernel::Pp: std::snprintf(name, sizeof name, "hrx::witness_pp_kernel"); break;
        case Kernel::Pmd: std::snprintf(name, sizeof name, "hrx::witness_pmd_kernel<%u, %s>", D, class_wide ? (sm ? "true, true, true" : "true, true, false") : li.pmd_fin ? "false, true, false" : "false, false, false"); break;
        case Kernel::Pm: std::snprintf(name, sizeof name, "hrx::witness_pm_kernel<%u, %s, %s, %s, %s, %s>", D, tf[li.gtab], tf[li.wide], tf[li.half], tf[sm], tf[li.byte]); break;
        case Kernel::Split: std::snprintf(name, sizeof name, "hrx::witness_split_kernel<%u, %u, %s>", D, li.byte ? 32u : 32u / D, tf[li.byte]); break;
        case Kernel::OneWave: std::snprintf(name, sizeof name, "hrx::witness_kernel<%u, %s, %s>", D, tf[(M % 8) == 0], tf[li.gtab]); break;
    }
    if (class_wide && sm) std::snprintf(line, sizeof line, "%s grid=%d waves=%d ring=%d sub-tiles=%u lds=%zu", name, li.grid, li.waves_per_wg, li.nslots, li.sm_bufs, li.lds_bytes);
    else std::snprintf(line, sizeof line, "%s grid=%d waves=%d ring=%d lds=%zu%s", name, li.grid, li.waves_per_wg, li.nslots, li.lds_bytes, li.dyn ? " groups=dynamic" : "");
    std::string out = line;
    if (li.kernel == Kernel::OneWave) {      // the one-wave kernel: strings per wave (64, 32 with kDbgGroups32, halved while the batch would leave CUs without a wave)
        std::snprintf(line, sizeof line, " gs=%u", li.gs);
        out += line;
    }
    if (li.spec_tiles) {
        std::snprintf(line, sizeof line, " chunked=%dx%d tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind", li.spec_chunks, li.spec_tiles);
        out += line;
    }
    return out;
}

extern "C" {

int describe_config(const DefsSet &s, const uint32_t dbg, const uint32_t tune, const bool mpc_on, int layout, size_t B, size_t M, int num_cus, char *out, size_t cap) {
    // HRX_LAYOUT_RECORD_PLANES: the launch hrx_witness_batch_device_planes makes (one def: described with its two row stripes); a config that takes no
    // planes is described as without them
    const size_t n_planes = (layout & HRX_LAYOUT_RECORD_PLANES) ? (s.defs.size() == 1 ? 2 : s.defs.size()) : 0;
    layout &= ~HRX_LAYOUT_RECORD_PLANES;
    BatchRoute r;
    std::string err;
    if (int rc = plan_batch_route(s, dbg, tune, mpc_on, layout, B, M, 0, num_cus, n_planes, false, r, err)) return fail(rc, err);
    const bool class_wide = r.kind == BatchRoute::Case::ClassWide || r.kind == BatchRoute::Case::ClassWideSm || r.kind == BatchRoute::Case::ClassWideGroups;
    std::string text;
    if (r.kind == BatchRoute::Case::ClassWideGroups || r.kind == BatchRoute::Case::GroupsOfThree) {
        text = "multi-pass, " + std::to_string(r.passes.size()) + " groups: ";
        for (const BatchRoute::Pass &ps : r.passes)
            text += "[defs " + std::to_string(ps.first_def) + ".." + std::to_string(ps.first_def + ps.set->defs.size() - 1) + ": " + launch_text(ps, class_wide, M) + "] ";
        text += r.merge_last ? "(the last pass merges the summaries) + hrx::witness_merge_status_kernel"
                             : class_wide || r.summary_mode ? "+ hrx::witness_combine_summary_kernel" : "+ hrx::witness_combine_kernel<true>";
    } else {
        text = launch_text(r.passes[0], class_wide, M);
    }
    if (r.transpose) text += " + hrx::transpose_pm_to_sm_kernel";
    std::snprintf(out, cap, "%s", text.c_str());
    return HRX_OK;
}

int hrx_describe_launch(const hrx_defs *defs, int layout, size_t B, size_t M, int num_cus, char *out, size_t cap) {
    if (!defs || !out || !cap) return fail(HRX_ERR_ARG, "NULL argument");
    if (!defs->s.finalized) return fail(HRX_ERR_STATE, "call hrx_defs_finalize first");
    if (num_cus < 1) return fail(HRX_ERR_ARG, "num_cus must be >= 1");
    const char *mpc = std::getenv("HRX_MP_COMBINE");      // (what hrx_ctx_create would read now)
    return describe_config(defs->s, debug_flags_from_env(), 0u, mpc && std::atoi(mpc) != 0, layout, B, M, num_cus, out, cap);
}

int hrx_ctx_describe_launch(const hrx_ctx *ctx, int layout, size_t B, size_t M, char *out, size_t cap) {
    if (!ctx || !out || !cap) return fail(HRX_ERR_ARG, "NULL argument");
    return describe_config(ctx->s, ctx->debug, ctx->tune, ctx->mp_combine, layout, B, M, ctx->num_cus > 0 ? ctx->num_cus : 256, out, cap);
}

}  // extern "C"
