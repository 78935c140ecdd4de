// hrx_plan.cpp — the launch planner: which kernel, table form and geometry serve a shape (plan_witness_launch and its kin), and which launches
// serve a whole witness call (plan_batch_route).  Host code only, no HIP call: launch_batch (hrx_api.cpp) executes a plan, describe_config
// (hrx_describe_api.cpp) prints one, tests/test_plan_golden_cpu.py holds every choice against a recorded sweep.
#include "hrx_plan.hpp"

#include <algorithm>

#include "../../include/hrx.h"
#include "hrx_lane.h"

namespace hrx {

// Which of the position-major kernel's stores are write-back instead of streaming.  All-streaming output is not the best this
// memory system does with a launch that writes more than the 256-MB Infinity Cache holds: with about 128 MiB of the records
// stored write-back (every k-th tile's) the bench line runs at 63-67 us in every process instead of 70 or 78 (NOTES_MEASUREMENTS.md §4.1:
// same-process and fresh-process A/Bs, tools/nt_mix_sweep.sh) and D = 3 at 65536 x 1024 B goes 0.72 -> 0.84.  Part of that is the
// cache absorbing lines that the NEXT launch overwrites (the bench re-writes its buffers every step); with outputs rotating over
// 4-8 buffer sets the policy is neutral (81-83 us either way, tools/rotating_outputs.py), and whoever consumes the rows next
// finds that share in the cache.  Not for launches whose whole footprint fits the cache (there streaming wins: 36.1 vs 38.0 us
// at M = 512), nor for the HALF kernel (cfg 5: 0.42 vs 0.43-0.45 ms), nor where k would exceed 8.  The string-major walker/storer
// kernel takes the same policy per 64-row block (cfg 2 string-major: 0.65 -> 0.71 of the peak).
uint32_t plan_nt_mix(const WitnessArgs &a, const LaunchInfo &li) {
    const bool pm = (a.layout & 1u) && li.kernel == Kernel::Pm && !li.half, sm_split = !(a.layout & 1u) && li.kernel == Kernel::Split;   // (the walker/storer kernel streams full lines too)
    if (!pm && !sm_split) return 0u;
    // The finisher's open-span rule (masked rows of a tile into which an open optimistic span reaches are written back, so that a repair merges in L2) pays where repairs happen — one-def
    // kernels: the bench line + 1.7 %, cfg 5 + 4-8 % — and costs where spans are long and DO end: headers3 65536 x 2048 0.687 with it against 0.721 without, regex2+3 0.745 against 0.749,
    // regex123 0.751 against 0.753 (tools/ab_policy.py on the release kernels, two leases, profiles/r05_probes/ab_policy.txt).  From two defs on the masked rows are streamed.
    const uint32_t flags = pm && a.D >= 2u ? kNtMixNoOpenSpan : 0u;
    const size_t rows = pm ? (size_t)a.M : (size_t)a.rec_pitch;   // string-major: the rows between consecutive strings
    const size_t rec_bytes = (size_t)a.B * rows * 4u * a.D, msk_bytes = (size_t)a.B * a.M * 2u;
    if (rec_bytes + msk_bytes < ((size_t)256 << 20)) return flags;
    const size_t k = (rec_bytes + ((size_t)128 << 20) - 1) / ((size_t)128 << 20);
    return (k < 2 ? 2u : k <= 8 ? (uint32_t)k : 0u) | flags;
}

void apply_plan(WitnessArgs &a, const LaunchInfo &li) {
    a.gs = li.gs;
    a.n_groups = li.n_groups;
    a.sm_no_touch = li.sm_no_touch;
    a.sm_bufs = li.sm_bufs;
}

static uint32_t groups_of_64(const WitnessArgs &a) { return (uint32_t)(((size_t)a.B + 63) / 64); }
static int grid_of(size_t need, size_t cap) { return need < cap ? (need < 1 ? 1 : (int)need) : (cap < 1 ? 1 : (int)cap); }

// A whole config of 4 .. 8 defs through the def-parallel kernel on the CLASS-WIDE tables (hrx_kernel_pmd.hip CW): position-major outputs, a.cw_image / a.table_bytes set.  One group per
// workgroup: D walkers + a combiner wave + a loader.  Same-lease A/B against the passes over groups of three
// defs, 65536 x 2048 / 1024 rows (tools/dn_bench.py, outputs equal bit for bit): D = 4 0.468 against 0.577 ms / 0.220 against 0.285; D = 5 0.581 against 0.637 / 0.293 against 0.319;
// D = 6 0.644 against 0.763 / 0.317 against 0.371; D = 7 0.797 against 0.922 / 0.415 against 0.458.  (With the last def's walker combining — the first version — four and five defs ran no
// faster than their two passes: the combiner, walk + D - 1 merges + reveal mask + masked rows per tile, set the pace of every group.)
bool plan_pmd_cw(const WitnessArgs &a, int num_cus, LaunchInfo &out) {
    out = LaunchInfo{};
    out.gs = 64;
    out.n_groups = groups_of_64(a);
    if (!(a.layout & 1u) || !a.cw_image || a.D < 4u || a.D > 8u || (a.debug & kDbgNoDefParallel)) return false;
    const int fin = 1;      // a combiner wave of its own: D + 2 waves (seven and eight defs: nine and ten waves at 168 VGPRs, the combiner's merge loop rolled)
    for (int ns = 4; ns >= 2; --ns) {
        const size_t lds = a.table_bytes + pmd_group_bytes((int)a.D + fin, ns);     // the publishing walkers' areas
        if (lds > kLdsLimit) continue;
        out.kernel = Kernel::Pmd;
        out.wide = 1;
        out.waves_per_wg = (int)a.D + 1 + fin;
        out.nslots = ns;
        out.lds_bytes = lds;
        out.grid = grid_of(out.n_groups, (size_t)num_cus);
        return true;
    }
    return false;
}

// ... with STRING-MAJOR outputs straight out of the launch (four and five defs, rows in multiples of 16): + a storer wave per group, two LDS sub-tile buffers of [64 strings][D][16 rows]
// and the masked rows' 8-KiB transpose buffer (hrx_kernel_pmd.hip SMO)
bool plan_pmd_cw_sm(const WitnessArgs &a, int num_cus, LaunchInfo &out) {
    out = LaunchInfo{};
    out.gs = 64;
    out.n_groups = groups_of_64(a);
    if ((a.layout & 1u) || !a.cw_image || a.D < 4u || a.D > 5u || (a.M % 16u) != 0u || (a.debug & kDbgNoDefParallel)) return false;
    if ((size_t)a.rec_pitch * a.D * 4u * 64u > 0xffffffffull) return false;      // the storer's 32-bit lane offsets span 64 strings' records
    for (int nbuf = 3; nbuf >= 2; --nbuf)      // three sub-tile buffers where LDS has room (four defs): 0.691 against 0.712 ms per 65536 x 2048, the same at x 1024 (profiles/r05_probes/sm_out_of_the_launch.txt)
        for (int ns = 4; ns >= (nbuf == 3 ? 3 : 2); --ns) {
            const size_t lds = a.table_bytes + pmd_group_bytes((int)a.D + 1, ns) + (size_t)nbuf * 64 * (16 * (size_t)a.D + 4) * 4 + 8192;
            if (lds > kLdsLimit) continue;
            out.sm_bufs = (uint32_t)nbuf;
            out.kernel = Kernel::Pmd;
            out.wide = 1;
            out.waves_per_wg = (int)a.D + 3;
            out.nslots = ns;
            out.lds_bytes = lds;
            out.grid = grid_of(out.n_groups, (size_t)num_cus);
            return true;
        }
    return false;
}

// ---------------------------------------------------------------------------------------------
// plan_witness_launch: a ladder of branches, each a function below that either fills `out` and returns true or leaves the next one its turn.
// ---------------------------------------------------------------------------------------------
struct PlanIn {             // what one pass over the ladder reads
    const WitnessArgs &a;
    int num_cus;
    uint32_t debug;         // a.debug; the walk over the chunks of a chunked launch is planned with bits of its own
    uint32_t n_groups;      // groups of 64 strings; the walk over chunks: x chunks per string
    bool planes;            // the records go into planes of their own (WitnessArgs::rec_planes)
    bool may_chunk;         // false: a pass of a multi-pass config, or the walk over the chunks of a chunked launch being planned (not chunked again)
    bool gtab;              // the fused table is walked out of global memory ...
    size_t table_bytes;     // ... and then takes no LDS: 0 in the budgets below
    bool pm() const { return (a.layout & 1u) != 0; }
    size_t cus(size_t k = 1) const { return (size_t)num_cus * k; }
};

// The ring kernels' search, once: "as few walker pairs per workgroup as the batch needs, the deepest ring that fits, grid = min(need, CUs x per-CU cap)".
// A branch states what differs: the bytes outside the pairs, a pair's bytes at a ring depth, the ring range, waves per pair, the per-CU wave cap and
// how the grid is capped.
// "As few pairs as the batch needs" spreads a small batch over the CUs — but never at the price of a second round (one_round): where the table leaves
// LDS for ONE workgroup per CU, 257-511 groups with one pair per workgroup ran twice as long as with two (pair-step kernel, 24576 x 32768 B: 2.1 vs 1.4 ms).
struct RingSpec {
    size_t fixed;                       // bytes outside the pairs: the table
    int ns_max, ns_min;                 // ring depths, the deepest that fits wins
    int wpp;                            // waves per pair
    int max_waves;                      // per CU
    enum Cap { kByWaves, kOnePerCu, kUpTo4PerCu } cap;   // workgroups per CU behind the grid: LDS and max_waves; one; LDS, at most four
    bool covering_start = false;        // start from the fewest pairs that COVER the groups (<=) instead of the fewest that leave no CU idle (<)
    bool one_round = true;
};
struct RingFit { int pairs, ns, grid; size_t lds; };

template <class PairBytes>
static bool fit_rings(const PlanIn &p, const RingSpec &s, PairBytes pair_bytes /* (ns) -> one pair's bytes */, RingFit &r) {
    auto lds_of = [&](int pairs, int *ns_out = nullptr) -> size_t {      // the deepest ring that fits `pairs` pairs; 0: none does
        for (int ns = s.ns_max; ns >= s.ns_min; --ns)
            if (s.fixed + (size_t)pairs * pair_bytes(ns) <= kLdsLimit) { if (ns_out) *ns_out = ns; return s.fixed + (size_t)pairs * pair_bytes(ns); }
        return 0;
    };
    auto per_cu_by_waves = [&](size_t lds, int pairs) -> size_t {
        size_t per_cu = lds ? kLdsLimit / lds : 0;
        if (per_cu * (size_t)(s.wpp * pairs) > (size_t)s.max_waves) per_cu = (size_t)s.max_waves / (size_t)(s.wpp * pairs);
        return per_cu < 1 ? 1 : per_cu;
    };
    int pairs = 4;
    while (pairs > 1 && (s.covering_start ? (size_t)p.n_groups <= p.cus(pairs - 1) : (size_t)p.n_groups < p.cus(pairs))) --pairs;
    for (; s.one_round && pairs < 4; ++pairs)
        if ((size_t)p.n_groups <= p.cus(pairs) * per_cu_by_waves(lds_of(pairs), pairs) || !lds_of(pairs + 1)) break;   // one round, or no room for another pair
    for (; pairs >= 1; --pairs) {
        r.lds = lds_of(pairs, &r.ns);
        if (!r.lds) continue;
        const size_t per_cu = s.cap == RingSpec::kByWaves ? per_cu_by_waves(r.lds, pairs) : s.cap == RingSpec::kOnePerCu ? 1 : std::min<size_t>(4, std::max<size_t>(1, kLdsLimit / r.lds));
        r.pairs = pairs;
        r.grid = grid_of(((size_t)p.n_groups + pairs - 1) / pairs, p.cus(per_cu));
        return true;
    }
    return false;
}

static void take_rings(LaunchInfo &out, Kernel k, const RingFit &r, int wpp) {
    out.kernel = k;
    out.gtab = out.wide = out.half = out.byte = 0;
    out.waves_per_wg = wpp * r.pairs;
    out.nslots = r.ns;
    out.lds_bytes = r.lds;
    out.grid = r.grid;
}

// position-major loader/walker kernel: from EIGHT groups per walker pair on, the pairs take their groups from a counter
// instead of a fixed stride — the walkers of odd XCDs run 8-17 % slower than those of even ones (NOTES_MEASUREMENTS.md §4.1), and with a
// fixed split the launch waits for them.  A group is the unit, so this only pays with many groups per pair: 2^20 x 2048 B
// (D = 2, 16 groups per pair) 4.68 -> 4.45 ms; with 4 groups per pair the last groups are drawn long before the fast pairs
// run dry (262144 x 2048 B: 1.188 vs 1.184 ms), and with 16-tile groups the loader's counter access — it waits for its loads
// in flight — costs more than the balance gains (262144 x 1024 B: 0.320 -> 0.334 ms).  Hence >= 8 groups per pair of >= 32 tiles.
static int want_dyn(const PlanIn &p, int grid, int pairs) {
    const size_t slots = (size_t)grid * (size_t)pairs;
    if (!p.pm() || (p.debug & kDbgNoDynamicGroups)) return 0;
    if (p.debug & kDbgForceDynamicGroups) return (size_t)p.n_groups > slots ? 1 : 0;
    return ((size_t)p.n_groups >= 8 * slots && (p.a.M + 63u) / 64u >= 32u) ? 1 : 0;
}

static bool plan_ladder(PlanIn p, LaunchInfo &out);

// tiles per chunk of a chunked launch of this shape; 0: not chunked
static uint32_t chunk_tiles(const PlanIn &p) {
    const WitnessArgs &a = p.a;
    const uint32_t ntiles = (a.M + 63u) / 64u;
    uint32_t tpc = 0;
    if (p.debug & kDbgForceSpec) {
        tpc = 4;
        while (tpc <= kSpecMaxChunkTiles && (ntiles % tpc != 0u || ntiles / tpc > kSpecMaxChunks)) tpc *= 2;
        if (tpc > kSpecMaxChunkTiles || ntiles / tpc < 2u) tpc = 0;
    } else if (ntiles >= 64u && (a.D == 1u ? (size_t)p.n_groups < p.cus(2) : (size_t)p.n_groups * 4u <= p.cus(a.D == 2u ? 7u : 6u))) {
        // below two groups per CU the sequential kernels run for one or two chains with most walker slots empty (32768-byte strings,
        // 20480 / 28672 strings: D = 1 2.07 / 2.20 ms against 1.05 / 1.41 chunked; D = 2 2.10 / 2.34 against 1.67 / 2.28; D = 3 2.77 / 2.79
        // against 2.37 / 3.23: tools/spec_threshold.sh); from two groups per CU on they are memory-bound and win   // (D = 2: the def-parallel kernel's chain is 1.8 ms per 32768 rows; chunked wins up to 1.25 groups per CU)
        tpc = 16;
        while (tpc <= kSpecMaxChunkTiles && (ntiles % tpc != 0u || ntiles / tpc > kSpecMaxChunks)) tpc *= 2;
        if (tpc > kSpecMaxChunkTiles) tpc = 0;
    }
    for (uint32_t d = 0; d < a.D && d < kMaxDefsPerLaunch; ++d)
        if (a.dc[d].n_rows > 255u) tpc = 0;          // (the scout keeps states as bytes, 0xff = none)
    return tpc && a.B <= kPmBlock && a.M % 64u == 0u ? tpc : 0u;
}

// ---- CHUNKED launch (hrx_kernel_spec.hip): a batch of at most one group per CU runs for as long as one string's dependent chain
// (n x 29-50 ns) with three quarters of the walker slots empty.  Cut every string into chunks of 16 tiles, find the chunks' start
// states (scout + compose) and walk the chunks as groups of their own: the chip is full again.  From two groups per CU on the
// sequential kernels are bound by the memory system anyway (32768 x 32768 B: 1.3 ms of traffic against 0.95 ms of chain).
static bool try_chunked(const PlanIn &p, LaunchInfo &out) {
    const WitnessArgs &a = p.a;
    if (!p.pm() || p.gtab || !p.may_chunk ||
        (p.debug & (kDbgNoSpec | kDbgForceHalf | kDbgForceByte | kDbgForceGlobalTable | kDbgForcePair | kDbgForceDefParallel))) return false;
    const uint32_t tpc = chunk_tiles(p);
    if (!tpc) return false;
    const uint32_t chunks = ((a.M + 63u) / 64u) / tpc;
    PlanIn walk = p;        // the walk over the chunks: the loader / walker / finisher kernel over n_groups x chunks virtual groups, planned here, launched by the caller
    walk.n_groups = p.n_groups * chunks;
    walk.may_chunk = false;
    walk.debug = (p.debug & ~kDbgForceSpec) | kDbgNoPair | kDbgNoDefParallel | kDbgNoSpec;
    LaunchInfo li = out;
    if (!plan_ladder(walk, li) || li.kernel != Kernel::Pm || li.half || li.byte || li.gtab) return false;
    out = li;
    out.spec_tiles = (int)tpc;
    out.spec_chunks = (int)chunks;
    out.gs = 64;
    out.n_groups = p.n_groups;      // the REAL groups; the launch walks n_groups x spec_chunks
    return true;
}

// ---- loader / walker / finisher kernel on the BYTE table (1-byte next states + the pair tags off the chain): one def of up
// to 256 states whose 4-byte table does not fit LDS (cfg 5).  Half the HALF table's LDS, which buys what that variant
// lacks: a finisher wave and a ring of more than one slot (its walker spent 46 % of its cycles in the tile-end work).
static bool try_pm_byte(const PlanIn &p, LaunchInfo &out) {
    const WitnessArgs &a = p.a;
    if (!(p.pm() && a.D == 1 && a.byte_image && !(p.debug & (kDbgNoByte | kDbgForceHalf)) &&
          ((p.gtab && !(p.debug & kDbgForceGlobalTable)) || (p.debug & kDbgForceByte)))) return false;
    RingFit r;
    if (!fit_rings(p, {a.byte_bytes, 4, 2, 3, 12, RingSpec::kByWaves}, [](int ns) { return pm_pair_bytes((size_t)ns, false, true); }, r)) return false;
    take_rings(out, Kernel::Pm, r, 3);
    out.byte = 1;
    out.dyn = want_dyn(p, r.grid, r.pairs);
    return true;
}

// ---- loader/walker kernel on the HALF table (2-byte entries): DFAs of up to 256 states whose 4-byte table does not
// fit LDS (cfg 5: 256 x 256 -> 128 KiB) stay LDS-resident instead of being walked out of L2 (kDbgForceHalf forces it)
static bool try_pm_half(const PlanIn &p, LaunchInfo &out) {
    const WitnessArgs &a = p.a;
    if (!(p.pm() && a.half_image && ((p.gtab && !(p.debug & kDbgForceGlobalTable)) || (p.debug & kDbgForceHalf)))) return false;
    RingFit r;
    if (!fit_rings(p, {a.half_bytes, 4, 1, 2, 8, RingSpec::kByWaves}, [](int ns) { return pm_pair_bytes((size_t)ns, true, false); }, r)) return false;
    take_rings(out, Kernel::Pm, r, 2);
    out.half = 1;
    out.dyn = want_dyn(p, r.grid, r.pairs);
    return true;
}

// ---- pair-step loader/walker kernel (hrx_kernel_pp.hip): position-major, one def whose PAIR table exists (few byte classes):
// two bytes per dependent lookup.  Table + per pair a ring of >= 2 slots of 8 KiB (pair indices + raw bytes).
// Only for batches that leave walker slots empty (< 4 groups per CU): there the launch lasts as long as one string's
// dependent chain and halving the chain wins (8192 x 32768 B: 1.14 vs 1.57 ms; 16384 x 1023 B: 51.5 vs 58.4 us;
// 32768: 54.9 vs 59.8 us).  A full chip (>= 4 groups per CU) is bound by the memory system, and the one-byte kernel,
// with fewer instructions per row, sits on the no-compute mix ceiling: 69.8 vs 73.8 us at 65536 x 1023 B, 131 vs 134 us
// at 131072 (same-process A/B, profiles/r02_ab_pair_vs_single.txt).
// As few pairs per workgroup as cover the batch in ONE round (small batches spread over the CUs); the 76-KiB table leaves room
// for one workgroup per CU, so "fewer pairs" must not mean "a second round" (24576 x 32768 B ran 2.1 ms with one pair per CU).
// This branch alone lowers `pairs` while the groups are COVERED (<=, the others: while a CU would stay idle, <) and has no one-round step of
// its own for that reason; whether the difference is wanted everywhere was never measured, so it stays.
static bool try_pp(const PlanIn &p, LaunchInfo &out) {
    const WitnessArgs &a = p.a;
    if (!(p.pm() && a.D == 1 && a.pair_image && ((size_t)p.n_groups < p.cus(4) || (p.debug & kDbgForcePair)) &&
          !(p.debug & (kDbgNoPair | kDbgForceNarrow | kDbgForceWide | kDbgForceHalf | kDbgForceGlobalTable)))) return false;
    RingSpec s{a.pair_bytes, 4, 2, 3, 12, RingSpec::kByWaves};
    s.covering_start = true;
    s.one_round = false;
    RingFit r;
    if (!fit_rings(p, s, [](int ns) { return pp_pair_bytes((size_t)ns); }, r)) return false;
    take_rings(out, Kernel::Pp, r, 3);   // walker + loader + finisher
    return true;
}

// ---- def-parallel loader/walker kernel (hrx_kernel_pmd.hip): position-major, D >= 2 on the WIDE table, batches of at
// most two groups per CU — one walker wave per def, so that a group advances at the single-def rate
static bool try_pmd_wide(const PlanIn &p, LaunchInfo &out) {
    const WitnessArgs &a = p.a;
    if (!(p.pm() && a.D >= 2 && a.wide_image && !p.gtab && !(p.debug & (kDbgNoDefParallel | kDbgForceNarrow | kDbgForceHalf | kDbgForceGlobalTable)) &&
          a.B <= kPmBlock &&   // one block of the position-major buffers (hrx_lane.h): its strides are the whole batch's
          ((size_t)p.n_groups <= p.cus(2) || (p.debug & kDbgForceDefParallel)))) return false;
    const int G = (size_t)p.n_groups <= p.cus() && !(p.debug & kDbgForceDefParallel) ? 1 : 2;
    // a combiner wave of its own (FIN): the last def's walker otherwise carries walk + D - 1 merges + reveal mask + masked rows (2.36 of cfg 4's 2.9 ms with every record store
    // compiled out).  kTunePmdFin* (hrx_ctx_set_option HRX_OPT_PMD_COMBINER_WAVE) forces it on / off; the default is what profiles/r06_probes/cfg4_fin_ab.txt measured.
    // Same lease, same input, cfg 4 (tools/planes_ab.py): interleaved records 2.78 ms without / 3.04 with the combiner wave; record planes 2.69 without / 2.53 with — where the records'
    // write stream is what bounds the launch, two more waves per CU only disturb it; where the planes spread it over the classes, the combiner's chain is the bound that is left.
    const bool fin = (a.tune & kTunePmdFinMask) == kTunePmdFinOn || ((a.tune & kTunePmdFinMask) == 0u && p.planes);
    for (int ns = 4; ns >= 2; --ns) {
        const size_t lds = p.table_bytes + (size_t)G * (fin ? pmd_fin_group_bytes((int)a.D, ns) : pmd_group_bytes((int)a.D, ns));
        if (lds > kLdsLimit) continue;
        out.kernel = Kernel::Pmd;
        out.wide = 1;
        out.pmd_fin = fin ? 1 : 0;
        out.waves_per_wg = G * ((int)a.D + 1 + (fin ? 1 : 0));
        out.nslots = ns;
        out.lds_bytes = lds;
        out.grid = grid_of(((size_t)p.n_groups + G - 1) / G, p.cus());
        return true;
    }
    return false;
}

// ---- loader/walker kernel: table + per pair a ring of up to 4 input tiles (4 KiB each).  Position-major outputs: walker + loader + finisher per
// pair (hrx_kernel_pm.hip), the loader finishes the tiles; at most one pair per SIMD (VGPRs).
// WIDE table: ~4x fewer instructions per row at D = 3; every D >= 2 batch takes it (same-box A/B
// with spill-free kernels: 1.20 vs 1.33 ms at 262144 x 2048 B, D = 2; 3.48 vs 4.59 ms at 32768 x 32768 B, D = 3).
// D = 1 gains nothing: its walk is LDS-latency-bound either way.
static bool try_pm(const PlanIn &p, LaunchInfo &out) {
    const WitnessArgs &a = p.a;
    const bool fin = p.pm();
    const int wpp = fin ? 3 : 2;
    RingFit r;
    if (!fit_rings(p, {p.table_bytes, 4, 2, wpp, 4 * wpp, RingSpec::kByWaves}, [fin](int ns) { return pm_pair_bytes((size_t)ns, false, fin); }, r)) return false;
    const int gtab = out.gtab;
    take_rings(out, Kernel::Pm, r, wpp);
    out.gtab = gtab;
    out.wide = (a.wide_image && !p.gtab && !(p.debug & kDbgForceNarrow) && (a.D >= 2 || (p.debug & kDbgForceWide))) ? 1 : 0;
    out.dyn = want_dyn(p, r.grid, r.pairs);   // (0 for the string-major D = 3 use of this kernel: want_dyn checks the layout)
    return true;
}

// ---- walker/storer kernel (hrx_kernel_sm.hip): string-major outputs, rows in multiples of 8, per pair a ring of >= 2 slots + the storer's LDS-DMA sink.
// On the BYTE table: one def of up to 256 states whose 4-byte table does not fit LDS (cfg 5; it used to take the position-major kernel + a transpose
// launch: 0.23 of peak); the storer's L2 warm-up costs that shape a second pass over the input (sm_no_touch), and its grid is one workgroup per CU.
// On the 4-byte table: D in {1,2}, up to four workgroups per CU where LDS holds them.
// (The ring depth used to be computed by division here and by a loop in the other branches: the deepest ring that fits, either way.)
static bool try_split(const PlanIn &p, bool byte_table, LaunchInfo &out) {
    const WitnessArgs &a = p.a;
    if (p.pm() || a.M % 8u != 0 || (p.debug & kDbgForceOneWave)) return false;
    if (byte_table ? !(a.D == 1 && a.byte_image && p.gtab && !(p.debug & (kDbgNoByte | kDbgForceHalf | kDbgForceGlobalTable))) : !((a.D == 1 || a.D == 2) && !p.gtab)) return false;
    const size_t slot = 64 * 128 + 64 * 8 + 64 * (byte_table || a.D == 1 ? 32 : 16), fixed = 16 + 256;
    RingFit r;
    if (!fit_rings(p, {byte_table ? a.byte16_bytes : p.table_bytes, 4, 2, 2, 8, byte_table ? RingSpec::kOnePerCu : RingSpec::kUpTo4PerCu}, [=](int ns) { return (size_t)ns * slot + fixed; }, r)) return false;
    const int gtab = byte_table ? 0 : out.gtab;
    take_rings(out, Kernel::Split, r, 2);
    out.gtab = gtab;
    out.byte = byte_table ? 1 : 0;
    out.sm_no_touch = byte_table ? 1u : 0u;
    return true;
}

// ---- one-wave-does-all kernel.  Group size: 64 strings per wave; smaller groups only for batches that would otherwise leave CUs without a wave
// (two half-empty waves per SIMD were measured slower than one full one: the walk is issue-bound, not latency-bound)
static bool plan_one_wave(const PlanIn &p, LaunchInfo &out) {
    const WitnessArgs &a = p.a;
    out.kernel = Kernel::OneWave;
    out.nslots = 0;
    uint32_t gs = 64;
    if (p.debug & kDbgGroups32) gs = 32;
    while (gs > 16 && ((size_t)a.B + gs - 1) / gs < p.cus()) gs >>= 1;
    out.gs = gs;
    out.n_groups = (uint32_t)(((size_t)a.B + gs - 1) / gs);
    const size_t per_wave = wave_stage_bytes((int)a.D, gs);
    int waves = 0;
    for (int w = 8; w >= 1; --w) {
        if (p.table_bytes + per_wave * w <= kLdsLimit) { waves = w; break; }
    }
    if (!waves) return false;
    // fewer waves per workgroup when the batch cannot feed every CU otherwise
    while (waves > 1 && (size_t)out.n_groups < p.cus(waves)) --waves;
    out.waves_per_wg = waves;
    out.lds_bytes = p.table_bytes + per_wave * waves;
    const size_t wgs_per_cu = kLdsLimit / out.lds_bytes < 1 ? 1 : kLdsLimit / out.lds_bytes;
    const size_t max_wg = 8 / (size_t)waves < 1 ? 1 : 8 / (size_t)waves;  // <= 8 waves per CU: 2 per SIMD at 157 VGPRs
    out.grid = grid_of(((size_t)out.n_groups + waves - 1) / waves, p.cus(wgs_per_cu > max_wg ? max_wg : wgs_per_cu));
    return true;
}

static bool plan_ladder(PlanIn p, LaunchInfo &out) {
    const WitnessArgs &a = p.a;
    out.gtab = out.wide = out.half = out.byte = out.dyn = out.spec_tiles = out.spec_chunks = 0;
    // DFAs whose fused table leaves no room for the per-wave LDS areas are walked out of global memory (L2-resident)
    const size_t min_stage = p.pm() ? pm_pair_bytes(2, false, true) : wave_stage_bytes((int)a.D, 16);
    p.gtab = a.table_bytes + min_stage > kLdsLimit || (p.debug & kDbgForceGlobalTable);
    p.table_bytes = p.gtab ? 0 : a.table_bytes;
    out.gtab = p.gtab ? 1 : 0;
    if (try_chunked(p, out) || try_pm_byte(p, out) || try_pm_half(p, out) || try_pp(p, out) || try_pmd_wide(p, out)) return true;
    // string-major D = 3 (no walker/storer kernel: its string-tiles are 128 bytes = 32 / 16 rows of 1 / 2 defs): the
    // loader/walker kernel with the lane's own string-major strides, 5x the one-wave kernel (NOTES_MEASUREMENTS.md §3.4)
    const bool sm3 = !p.pm() && a.D == 3 && a.M % 8u == 0 && !p.gtab && !(p.debug & kDbgForceOneWave);
    if (p.pm() || sm3) return try_pm(p, out);
    return try_split(p, true, out) || try_split(p, false, out) || plan_one_wave(p, out);
}

// planes: the records go into planes of their own; pass: a summary-writing or merging pass of a multi-pass config
static bool plan_launch(const WitnessArgs &a, bool planes, bool pass, int num_cus, LaunchInfo &out) {
    out = LaunchInfo{};
    out.gs = 64;
    out.n_groups = groups_of_64(a);
    return plan_ladder(PlanIn{a, num_cus, a.debug, out.n_groups, planes, !pass, false, 0}, out);
}

bool plan_witness_launch(const WitnessArgs &a, int num_cus, LaunchInfo &out) {
    return plan_launch(a, a.rec_planes[0] != nullptr, a.summary || a.merge_G || a.vs_init, num_cus, out);
}

// MATCH (hrx_kernel_match.hip).  The fused kernel walks one string per lane; it takes every batch of at most three defs except where the witness
// planner walks in chunks (few long strings: one lane per string would be chain-bound, ~1.2 ms at 8192 x 32768 against the chunked witness's 0.45).
// Table: the narrow one in LDS where it fits (kDbgForceNarrow / kDbgForceWide: this one — the WIDE table only speeds up the witness's record
// assembly, which the match does not do), else the HALF table (also where kDbgForceHalf or kDbgForceByte say so: the BYTE table's pair-hash tags serve
// the witness's finisher wave, the match walk has none), else the narrow table out of L2 (GTAB; kDbgForceGlobalTable).
bool plan_match_launch(const WitnessArgs &a, int num_cus, bool via_rows, MatchPlan &out) {
    out = MatchPlan{};
    if (via_rows || a.D < 1 || a.D > 3 || !a.table_image) return true;
    LaunchInfo li;
    WitnessArgs w = a;
    w.layout |= 1u;   // (the "via rows" witness launch is position-major)
    if (plan_witness_launch(w, num_cus, li) && li.spec_tiles) return true;
    const bool fits = a.table_bytes <= kLdsLimit, has_half = a.half_image != nullptr;
    if (a.debug & kDbgForceGlobalTable) out.gtab = 1;
    else if (has_half && (a.debug & (kDbgForceHalf | kDbgForceByte))) out.half = 1;
    else if (fits) {}
    else if (has_half) out.half = 1;
    else out.gtab = 1;
    out.fused = 1;
    out.lds_bytes = out.gtab ? 0 : out.half ? (((size_t)a.half_bytes + 15) & ~(size_t)15) : (((size_t)a.table_bytes + 15) & ~(size_t)15);
    // workgroups of 256 lanes, fewer where that would leave CUs without one (a workgroup stages the table once: no smaller than one wave)
    out.threads = (int)kMatchThreads;
    while (out.threads > 64 && ((size_t)a.B + out.threads - 1) / out.threads < (size_t)num_cus) out.threads /= 2;
    out.grid = (int)(((size_t)a.B + out.threads - 1) / out.threads);
    return true;
}

// MATCH, four to eight defs (hrx_kernel_match_wide.hip): the rule of hrx_plan.hpp.  The "chunked" test is plan_match_launch's, asked of the route that the
// via-rows call of this shape would launch (today no route of four and more defs chunks: its launches are the def-parallel kernel or passes)
bool plan_match_wide(const DefsSet &s, uint32_t debug, bool via_rows, bool option, int layout, size_t B, size_t M, int num_cus, MatchPlan &out) {
    const size_t D = s.defs.size(), lds = (s.cw_image.size() + 15) & ~(size_t)15;
    if (!option || via_rows || D < 4 || D > kMaxDefsPerLaunch || s.cw_image.empty() || lds > kLdsLimit || layout != HRX_LAYOUT_STRING_MAJOR) return false;
    BatchRoute route;
    std::string err;
    if (plan_batch_route(s, debug, 0u, false, HRX_LAYOUT_POSITION_MAJOR, B, M, 0, num_cus, 0, false, route, err) != HRX_OK) return false;
    for (const BatchRoute::Pass &ps : route.passes)
        if (ps.li.spec_tiles) return false;
    out = MatchPlan{};
    out.fused = 1;
    // defs a sweep walks side by side: four (the fastest of 1, 2 and 4 at one wave per SIMD, where the walk is chain-latency bound, at four and at eight defs);
    // one by one at four defs for batches of more than a wave per SIMD (occupancy 2: 1.72 against 2.22 ms at 262144 x 1024).  DESIGN.md §16
    out.wide = D == 4 && B > (size_t)num_cus * kMatchThreads ? 1 : 4;
    out.lds_bytes = lds;
    out.threads = (int)kMatchThreads;
    out.grid = (int)((B + kMatchThreads - 1) / kMatchThreads);       // (persistent lanes: the launch caps it at what the device holds at once)
    return true;
}

// ---------------------------------------------------------------------------------------------
// a launch's table fields, and the route of a witness call
// ---------------------------------------------------------------------------------------------
SetImages host_images(const DefsSet &s, bool class_wide) {
    SetImages im;
    if (class_wide) { im.cw = s.cw_image.empty() ? nullptr : s.cw_image.data(); return im; }
    im.table = s.table_image.empty() ? nullptr : s.table_image.data();
    im.wide = s.wide_image.empty() ? nullptr : s.wide_image.data();
    im.half = s.half_image.empty() ? nullptr : s.half_image.data();
    im.pair = s.pair.image.empty() ? nullptr : s.pair.image.data();
    im.byte = s.byte.image.empty() ? nullptr : s.byte.image.data();
    return im;
}

WitnessArgs witness_args_of(const DefsSet &s, const SetImages &im) {
    WitnessArgs a{};
    a.D = (uint32_t)s.defs.size();
    if (im.cw) {
        a.cw_image = im.cw; a.cw_lut_off = s.cw_lut_off; a.table_bytes = (uint32_t)s.cw_image.size();
        for (uint32_t d = 0; d < a.D && d < kMaxDefsPerLaunch; ++d) a.dc[d] = s.cw_consts[d];
        return a;
    }
    a.table_image = im.table; a.table_bytes = (uint32_t)(s.table_image.size() * 4);
    a.wide_image = im.wide;
    a.half_image = im.half; a.half_bytes = (uint32_t)(s.half_image.size() * 2);
    a.pair_image = im.pair; a.pair_bytes = s.pair.bytes; a.pair_classes = s.pair.n_classes;
    a.pair_blk_bytes = s.pair.blk_bytes; a.pair_lut_off = s.pair.lut_off;
    a.byte_image = im.byte; a.byte_bytes = s.byte.bytes; a.byte_ptab_off = s.byte.ptab_off; a.byte_mul_a4 = s.byte.mul_a * 4; a.byte_mul_b4 = s.byte.mul_b * 4; a.byte_slot_mask4 = (s.byte.slots - 1u) * 4u;
    a.byte_dead = s.byte.dead;
    a.byte_rows_bytes = s.byte.n_rows * 256u; a.byte16_bytes = s.byte.bytes16; a.byte16_ptab_off = s.byte.ptab16_off;
    a.byte_one_id = (s.defs.size() == 1 && s.defs[0].substrs.size() == 1 && s.consts[0].substr_id_offset >= 1 && s.consts[0].substr_id_offset <= 63) ? s.consts[0].substr_id_offset : 0u;
    for (uint32_t d = 0; d < a.D && d < kMaxDefsPerLaunch && d < s.consts.size(); ++d) a.dc[d] = s.consts[d];
    return a;
}

namespace {
struct ShapeIn {
    const DefsSet &s;
    uint32_t debug, tune;
    size_t B, M, rec_pitch, n_planes;
    int num_cus;
};
const char *const kNoFit = "tables + staging do not fit the 160 KiB LDS";

WitnessArgs shape_args(const ShapeIn &in, const DefsSet &set, bool class_wide, int layout) {
    WitnessArgs a = witness_args_of(set, host_images(set, class_wide));
    a.layout = (uint32_t)layout; a.B = (uint32_t)in.B; a.M = (uint32_t)in.M;
    a.rec_pitch = (uint32_t)((layout & 1) ? in.M : in.rec_pitch);
    a.debug = in.debug; a.tune = in.tune;
    return a;
}

// one launch over `set` (a config of up to kMaxDefsPerPass defs, or one group of a larger one); pass: a summary-writing or merging pass of a
// multi-pass config, which is the loader / walker / finisher kernel: no pair-step or def-parallel variant, no HALF table, not chunked
int plan_set(const ShapeIn &in, const DefsSet &set, uint32_t first_def, int layout, bool pass, BatchRoute &out, std::string &err) {
    WitnessArgs a = shape_args(in, set, false, layout);
    BatchRoute::Pass ps{&set, first_def, layout, in.debug, 0u, LaunchInfo{}};
    // one def in two row stripes: the loader / walker / finisher kernel writes them (not the pair-step kernel, and not in chunks:
    // a chunk's first tile is not a stripe boundary in general, and the chunked launch's repair reads whole planes)
    if (in.n_planes && in.n_planes == 2 * (size_t)a.D) { ps.rec_stripes = 2; ps.debug |= kDbgNoPair | kDbgNoSpec; }
    if (pass) ps.debug |= kDbgNoPair | kDbgNoDefParallel;
    a.debug = ps.debug;
    if (!plan_launch(a, in.n_planes != 0, pass, in.num_cus, ps.li)) { err = kNoFit; return HRX_ERR_BOUNDS; }
    if (pass && ps.li.half) {   // (a group of one big DFA: walk its 4-byte table out of L2 instead)
        a.debug = ps.debug |= kDbgForceGlobalTable;
        if (!plan_launch(a, in.n_planes != 0, pass, in.num_cus, ps.li)) { err = kNoFit; return HRX_ERR_BOUNDS; }
    }
    if (pass && ps.li.kernel != Kernel::Pm) { err = "multi-pass: the planner did not pick the position-major loader/walker kernel"; return HRX_ERR_STATE; }
    out.passes.push_back(ps);
    return HRX_OK;
}

// a def-parallel launch on the CLASS-WIDE tables of `set` (the config, or one of its CW groups)
bool plan_cw(const ShapeIn &in, const DefsSet &set, uint32_t first_def, int layout, BatchRoute &out) {
    const WitnessArgs a = shape_args(in, set, true, layout);
    BatchRoute::Pass ps{&set, first_def, layout, in.debug, 0u, LaunchInfo{}};
    if (!((layout & 1) ? plan_pmd_cw(a, in.num_cus, ps.li) : plan_pmd_cw_sm(a, in.num_cus, ps.li))) return false;
    out.passes.push_back(ps);
    return true;
}
// up to kMaxDefsPerPass defs: one launch.
// String-major outputs of a DFA whose 4-byte table does not fit LDS (cfg 5): the string-major kernels would walk it out of global
// memory (0.21 of peak); the BYTE / HALF table kernels are position-major — run them into context scratch and turn the rows around
// (one def with a BYTE image has a string-major kernel of its own: the walker/storer kernel on that table)
int route_one_launch(const ShapeIn &in, int layout, BatchRoute &out, std::string &err) {
    const DefsSet &s = in.s;
    const bool byte_split = !s.byte.image.empty() && !(in.debug & (kDbgNoByte | kDbgForceHalf));
    out.transpose = layout == HRX_LAYOUT_STRING_MAJOR && in.M % 8 == 0 && !byte_split && (!s.byte.image.empty() || !s.half_image.empty()) &&
                    s.table_image.size() * 4 + wave_stage_bytes((int)s.defs.size(), 16) > kLdsLimit;
    if (out.transpose) out.layout = HRX_LAYOUT_POSITION_MAJOR;
    return plan_set(in, s, 0, out.layout, false, out, err);
}

// The whole config in ONE def-parallel launch on its CLASS-WIDE tables, where they exist (cw_whole); also decides whether the passes that serve the config
// otherwise run through the transposer.
bool route_class_wide(const ShapeIn &in, bool cw_whole, int layout, int pm_layout, BatchRoute &out) {
    // four and five defs, string-major outputs, rows in multiples of 16: the def-parallel launch writes the caller's [B][pitch][D] records and [B][pitch] masked rows itself — its walkers'
    // quads meet in LDS sub-tiles, a storer wave writes each string's 16 rows x D records as one run (hrx_kernel_pmd.hip SMO) — instead of position-major scratch + the transposer
    out.kind = BatchRoute::Case::ClassWideSm;
    if (layout == HRX_LAYOUT_STRING_MAJOR && cw_whole && plan_cw(in, in.s, 0, layout, out)) return true;
    // string-major outputs (rows in multiples of 8): the passes and the combine run position-major into context scratch and
    // transpose_pm_to_sm_kernel turns the rows around (hrx_kernel_tp.hip: 3.7 -> ~1 ms at D = 5, 65536 x 1024 rows); other row counts keep the
    // copy-mode combine (per-lane 4-byte stores)
    out.transpose = !(layout & HRX_LAYOUT_POSITION_MAJOR) && in.M % 8 == 0;
    if (out.transpose) out.layout = pm_layout;
    // 4 .. 8 defs whose CLASS-WIDE tables exist (every def <= 32 byte classes): ONE def-parallel launch walks all defs — one walker wave per def and a combiner wave
    // (hrx_kernel_pmd.hip CW) — instead of passes over groups of three with summaries in between: no second read of the input, no 80-byte tile summaries written and read back
    out.kind = BatchRoute::Case::ClassWide;
    return (out.layout & HRX_LAYOUT_POSITION_MAJOR) && cw_whole && plan_cw(in, in.s, 0, out.layout, out);
}

// more than eight defs, every def of at most 32 byte classes: passes over CW GROUPS of 4 .. 8 defs (DefsSet::cw_groups), each ONE def-parallel launch that writes its defs' planes of the
// caller's records and a tile summary; the combine launch forms what needs all defs of a row.  D = 16: two passes instead of six, D = 32: four instead of eleven.
bool route_class_wide_groups(const ShapeIn &in, BatchRoute &out) {
    out.kind = BatchRoute::Case::ClassWideGroups;
    if (!(out.layout & HRX_LAYOUT_POSITION_MAJOR) || in.s.cw_groups.empty() || (in.debug & kDbgNoDefParallel)) return false;
    size_t g = 0;
    while (g < in.s.cw_groups.size() && plan_cw(in, in.s.cw_groups[g], in.s.cw_group_first[g], out.layout, out)) ++g;
    if (g < in.s.cw_groups.size()) out.passes.clear();
    return g == in.s.cw_groups.size();
}

// one ordinary launch per group of three.  Position-major outputs: the passes write the caller's record planes themselves and a tile summary each; up to kMaxMergeGroups + 1 groups:
// the LAST pass reads the earlier groups' summaries itself and writes the final masked rows, a one-thread-per-string launch merges the status words (HRX_MP_COMBINE=1: the separate
// combine launch, as with more groups).  Else: group-private records, position-major, and the copy-mode combine.
int route_groups_of_three(const ShapeIn &in, bool mp_combine, int pm_layout, BatchRoute &out, std::string &err) {
    const bool pm_out = (out.layout & HRX_LAYOUT_POSITION_MAJOR) != 0;
    out.kind = BatchRoute::Case::GroupsOfThree;
    out.summary_mode = pm_out;
    out.merge_last = pm_out && in.s.groups.size() - 1 <= kMaxMergeGroups && !mp_combine;
    for (size_t g = 0; g < in.s.groups.size(); ++g)
        if (int rc = plan_set(in, in.s.groups[g], in.s.group_first[g], pm_out ? out.layout : pm_layout, pm_out, out, err)) return rc;
    return HRX_OK;
}
}  // namespace

int plan_batch_route(const DefsSet &s, uint32_t debug, uint32_t tune, bool mp_combine, int layout, size_t B, size_t M, size_t rec_pitch, int num_cus,
                     size_t n_planes, bool strict_planes, BatchRoute &out, std::string &err) {
    out = BatchRoute{};
    out.layout = layout;
    const bool cw_whole = !s.cw_image.empty() && !mp_combine;
    if (n_planes && !s.groups.empty() && !cw_whole) {
        if (strict_planes) { err = "record planes: configs that run as one launch (up to three defs, or four to eight defs of at most 32 byte classes each)"; return HRX_ERR_ARG; }
        n_planes = 0;
    }
    ShapeIn in{s, debug, tune, B, M, rec_pitch ? rec_pitch : M, n_planes, num_cus};
    if (s.groups.empty()) return route_one_launch(in, layout, out, err);
    if (s.groups.size() > kMaxGroups) { err = "too many def groups"; return HRX_ERR_BOUNDS; }
    const int pm_layout = HRX_LAYOUT_POSITION_MAJOR | (layout & HRX_LAYOUT_INPUT_POSITION_MAJOR);
    if (route_class_wide(in, cw_whole, layout, pm_layout, out)) return HRX_OK;
    if (in.n_planes && strict_planes) { err = "record planes: the one-launch def-parallel path does not fit this config"; return HRX_ERR_BOUNDS; }
    in.n_planes = 0;
    return route_class_wide_groups(in, out) ? HRX_OK : route_groups_of_three(in, mp_combine, pm_layout, out, err);
}

// The chunk of the chunked verify (hrx_ctx_verify_chunk_rows): the fewest chunks K that give every SIMD of the device two waves — ceil(B / 64) K >= 8 CUs
// (the one- to three-def kernels hold two waves per SIMD) — but never so many that a chunk falls below kVerifyChunkFloor rows (K <= M / floor):
// a chunk pays for the two rows it reads beside its own, for one summary and for its share of the stitch launch.  The rows are cut evenly, in multiples of
// 64.  The floor is measured, not derived (tools/verify_bench.py --floor-sweep, NOTES_MEASUREMENTS.md §20).  A result >= M: one chunk, the unchunked launch
// is the better call.
size_t plan_verify_chunk_rows(size_t B, size_t M, int num_cus) {
    if (B == 0 || M == 0) return M;
    const size_t groups = (B + 63) / 64, want = (size_t)8 * (size_t)(num_cus > 0 ? num_cus : 256);
    size_t K = groups >= want ? 1 : (want + groups - 1) / groups;
    K = std::min(K, std::max<size_t>(1, M / kVerifyChunkFloor));
    return ((M + K - 1) / K + 63) / 64 * 64;
}

}  // namespace hrx
