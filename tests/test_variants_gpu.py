"""The variant matrix: every kernel variant the planner can be forced into (HRX_DEBUG_FLAGS, HRX_OPT_PMD_COMBINER_WAVE, HRX_MP_COMBINE), run on the
edge-case definitions and batches of tests/fuzz_defs.py, every output buffer allocated here with a poisoned guard behind it.

Per row and seed: describe_launch names the variant the row forces (a silently ignored flag fails, it does not pass on the default kernel); status words,
records and masked rows equal OracleDefs.witness_batch bit for bit; no byte behind a buffer or in a pitch gap changes.  Per row: the seeds together hold
strings of every status the row can produce, an accepted state and a nonzero masked row, and one flipped bit of a downloaded record is reported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fuzz_defs as fd
from oracle_lib import OracleDefs

pytestmark = pytest.mark.gpu

NO_HOST = 0x20000000          # kDbgNoHost (csrc/hrx_kernel.hpp)
POISON = 0xA5
GUARD = 4096                  # bytes behind every output buffer
SEEDS = (0, 1, 2, 3, 4, 16)

# Per row: the entry point (sm: witness_batch, odd seeds into pitched buffers; pm: witness_batch_position_major from both input layouts, then
# witness_batch_planes — record planes at D >= 2, two row stripes at D = 1), the HRX_DEBUG_FLAGS bits, the HRX_OPT_PMD_COMBINER_WAVE option (option=(1, v)),
# HRX_MP_COMBINE, the shapes at which the variant is reached, the launch describe_launch must name ({D}: defs, {m8}: M % 8 == 0, {g}: 32 / D),
# fr: fr_columns against F::from of the oracle's columns on the row's fr_case ("D1": a one-def case, so that the row stripes are checked too),
# planes=False: the library refuses record planes for the config, and writes nothing.  Dynamic groups and the one-wave kernel's full group sizes need
# more groups than these small batches make: those rows repeat their batches (Shape.min_batch).
ROWS = [
    # ---- string-major outputs (witness_batch; odd seeds into pitched buffers)
    dict(id="sm-split-4byte", entry="sm", flags=0, shape=fd.Shape(1, 2, m="m16"), expect=r"witness_split_kernel<{D}, {g}, false>", fr="any"),
    dict(id="sm-split-byte", entry="sm", flags=0, shape=fd.Shape(1, 1, "big", m="m16", ids=("ids_62", "ids_63")), expect=r"witness_split_kernel<1, 32, true>"),
    # (the one-wave kernel halves its group size while the batch would leave CUs without a wave: gs64 / gs32 need >= 256 groups of 64 / 32 strings)
    dict(id="sm-one-wave-gs64", entry="sm", flags=0x10000, shape=fd.Shape(1, 2, m_max=80, min_batch=16384), expect=r"witness_kernel<{D}, {m8}, false> .* gs=64$"),
    dict(id="sm-one-wave-gs32", entry="sm", flags=0x30000, shape=fd.Shape(1, 2, m_max=80, min_batch=16384), expect=r"witness_kernel<{D}, {m8}, false> .* gs=32$"),
    dict(id="sm-global", entry="sm", flags=0x40000, shape=fd.Shape(1, 3, ids=("ids_62", "ids_63", "ids_64")), expect=r"witness_kernel<{D}, {m8}, true>"),
    dict(id="sm-via-pm-half", entry="sm", flags=0x8000, shape=fd.Shape(1, 1, "big", m="m8"),
         expect=r"witness_pm_kernel<1, false, false, true, \w+, false> .* \+ hrx::transpose_pm_to_sm_kernel"),
    # ---- position-major outputs, both input layouts
    dict(id="pm-narrow", entry="pm", flags=0x80000, shape=fd.Shape(1, 3), seeds=(0, 1, 2, 3, 4, 9),
         expect=r"witness_pm_kernel<{D}, false, false, false, false, false>", fr="D1"),
    dict(id="pm-wide", entry="pm", flags=0x200000 | 0x2000000, shape=fd.Shape(1, 3, ascii=True), expect=r"witness_pm_kernel<{D}, false, true, false, false, false>"),
    dict(id="pm-half", entry="pm", flags=0x400000, shape=fd.Shape(1, 1, "big"), expect=r"witness_pm_kernel<1, false, false, true, false, false>"),
    dict(id="pm-half-small", entry="pm", flags=0x400000, shape=fd.Shape(2, 3), expect=r"witness_pm_kernel<{D}, false, false, true, false, false>"),
    dict(id="pm-byte", entry="pm", flags=0x2000 | 0x8000000, shape=fd.Shape(1, 1, "big", ids=("ids_62", "ids_63")), expect=r"witness_pm_kernel<1, false, false, false, false, true>"),
    dict(id="pm-global", entry="pm", flags=0x40000, shape=fd.Shape(1, 3, ids=("ids_65", "ids_sum_255")), seeds=(0, 1, 2, 3, 4, 22), expect=r"witness_pm_kernel<{D}, true, false, false, false, false>"),
    dict(id="pm-dynamic-groups", entry="pm", flags=0x1000 | 0x80000, shape=fd.Shape(1, 3, m_max=144, min_batch=70000),
         expect=r"witness_pm_kernel<{D}, false, false, false, false, false> .*groups=dynamic$"),
    dict(id="pm-static-groups", entry="pm", flags=0x800 | 0x80000, shape=fd.Shape(1, 3), expect=r"witness_pm_kernel<{D}, false, false, false, false, false> grid=\d+ waves=\d+ ring=\d+ lds=\d+$"),
    dict(id="pm-pair-step", entry="pm", flags=0x40000000, shape=fd.Shape(1, 1, "pair"), expect=r"witness_pp_kernel"),
    dict(id="pm-def-parallel", entry="pm", flags=0x4000000, option=(1, 2), shape=fd.Shape(2, 3, ascii=True, s_max=12),
         expect=r"witness_pmd_kernel<{D}, false, false, false>"),
    dict(id="pm-def-parallel-combiner", entry="pm", flags=0x4000000, option=(1, 1), shape=fd.Shape(2, 3, ascii=True, s_max=12),
         expect=r"witness_pmd_kernel<{D}, false, true, false>", fr="any"),
    dict(id="pm-class-def-parallel", entry="pm", flags=0, shape=fd.Shape(4, 8, s_max=12), expect=r"^hrx::witness_pmd_kernel<{D}, true, true, false>"),
    dict(id="sm-class-def-parallel-subtiles", entry="sm", flags=0, shape=fd.Shape(4, 5, m="m16", s_max=12, m_max=64),
         expect=r"^hrx::witness_pmd_kernel<{D}, true, true, true> .*sub-tiles"),
    dict(id="pm-multi-pass-merge", entry="pm", flags=0x2000000, shape=fd.Shape(4, 7), expect=r"^multi-pass.*the last pass merges the summaries", planes=False),
    dict(id="pm-multi-pass-combine", entry="pm", flags=0x2000000, mp_combine=True, shape=fd.Shape(4, 7), expect=r"^multi-pass.*\+ hrx::witness_combine_summary_kernel", planes=False),
    # ---- string-major outputs of three and more defs: what an unmodified string-major caller of such a config runs.  Three defs at M % 8 == 0: the
    # loader/walker kernel's own string-major form.  More: M % 8 != 0 is the copy-mode combine behind passes over groups of three (its records and masked
    # rows are per-lane stores at the caller's pitches, its take-backs a store loop of data-dependent length); M % 8 == 0 runs position-major into context
    # scratch and through the transposer, behind each of its producers: the class-wide def-parallel launch (four and five defs only off M % 16 == 0, where
    # the sub-tile form takes over), class-wide groups with the summary combine, groups of three merged by the last pass or combined; and behind a HALF
    # walk of two and three defs.  The transposer's tile is 128 / 64 / 32 / 16 rows at D = 1 / 2 / 3..9 / >= 10: the m8x and m8 pools hold row counts below
    # a tile, one octet on either side of its border, and partial last tiles.  The two-blocks rows repeat their batches past one position-major block of
    # 65536 strings (the last group of the second block is partial)
    dict(id="sm-three-defs-loader-walker", entry="sm", flags=0, shape=fd.Shape(3, 3, m="m8"), expect=r"^hrx::witness_pm_kernel<3, false, \w+, false, true, false> (?!.*transpose)"),
    dict(id="sm-multi-pass-copy-combine", entry="sm", flags=0, shape=fd.Shape(4, 8, m="odd8"), expect=r"^multi-pass.*\+ hrx::witness_combine_kernel<true>"),
    dict(id="sm-class-wide-transpose", entry="sm", flags=0, shape=fd.Shape(4, 8, m="m8x", s_max=12), seeds=(0, 1, 2, 4, 9, 18),
         expect=r"^hrx::witness_pmd_kernel<{D}, true, true, false> .* \+ hrx::transpose_pm_to_sm_kernel$"),
    # (seeds 21 and 23: 8 rows at ten defs and 16 at twelve, the 16-row tile's first sizes, with more than one string)
    dict(id="sm-class-wide-groups-transpose", entry="sm", flags=0, shape=fd.Shape(9, 12, m="m8", s_max=12), seeds=(0, 1, 2, 3, 4, 16, 21, 23),
         expect=r"^multi-pass.*witness_pmd_kernel<.*\+ hrx::witness_combine_summary_kernel \+ hrx::transpose_pm_to_sm_kernel$"),
    dict(id="sm-multi-pass-merge-transpose", entry="sm", flags=0x2000000, shape=fd.Shape(4, 7, m="m8"),
         expect=r"^multi-pass.*the last pass merges the summaries.* \+ hrx::transpose_pm_to_sm_kernel$"),
    dict(id="sm-multi-pass-combine-transpose", entry="sm", flags=0x2000000, mp_combine=True, shape=fd.Shape(4, 7, m="m8"),
         expect=r"^multi-pass.*\+ hrx::witness_combine_summary_kernel \+ hrx::transpose_pm_to_sm_kernel$"),
    # (the HALF image holds at most 256 states over all defs: no 255-state def beside others, and small other defs)
    dict(id="sm-via-pm-half-defs", entry="sm", flags=0x8000, shape=fd.Shape(2, 3, "big", m="m8", big_kinds=("big_total", "big_partial"), s_max=12), seeds=(0, 2, 3, 4, 7, 19, 24),
         expect=r"witness_pm_kernel<{D}, false, false, true, \w+, false> .* \+ hrx::transpose_pm_to_sm_kernel$"),
    # (batches of at most 129 strings: fewer groups of 32 than CUs)
    dict(id="sm-one-wave-gs16", entry="sm", flags=0x10000, shape=fd.Shape(1, 3), expect=r"witness_kernel<{D}, {m8}, false> .* gs=16$"),
    dict(id="sm-class-wide-transpose-two-blocks", entry="sm", flags=0, shape=fd.Shape(6, 6, m="m8", s_max=12, m_max=40, min_batch=65600),
         expect=r"^hrx::witness_pmd_kernel<6, true, true, false> .* \+ hrx::transpose_pm_to_sm_kernel$"),
    dict(id="sm-copy-combine-two-blocks", entry="sm", flags=0, shape=fd.Shape(6, 6, m="odd8", m_max=40, min_batch=65600),
         expect=r"^multi-pass.*\+ hrx::witness_combine_kernel<true>"),
]
ROW_IDS = [r["id"] for r in ROWS]


def row_expect(row, D, M):
    return row["expect"].format(D=D, m8="true" if M % 8 == 0 else "false", g=32 // D)


def row_layouts(row):
    return [0] if row["entry"] == "sm" else [1, 3]


def applicable_edges(row):
    """the edge cases of fuzz_defs that the row's shape admits"""
    sh = row["shape"]
    e = set(fd.DEF_EDGES) | set(fd.UNDEF_EDGES) | set(fd.BYTE_EDGES) | set(fd.LEN_EDGES) | set(sh.ids)
    if sh.states == "big":
        e |= set(sh.big_kinds)
    if sh.states == "pair":
        e.add("few_classes")
    if sh.m_max <= 64:
        e.discard("undef_64")
    if sh.m_max <= 63:
        e.discard("undef_63")
    return e


def make_config(hra, row, case, device):
    """(config, oracle defs) with the row's flags, option and HRX_MP_COMBINE in force (HRX_DEBUG_FLAGS / HRX_MP_COMBINE are read when the context is made)"""
    os.environ["HRX_DEBUG_FLAGS"] = str(row["flags"] | NO_HOST)
    if row.get("mp_combine"):
        os.environ["HRX_MP_COMBINE"] = "1"
    else:
        os.environ.pop("HRX_MP_COMBINE", None)
    try:
        defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
        cfg = hra.RegexVerifyConfig.configure(case.M, defs, device=device)
    finally:
        os.environ.pop("HRX_DEBUG_FLAGS", None)
        os.environ.pop("HRX_MP_COMBINE", None)
    if row.get("option"):
        cfg.set_option(*row["option"])
    return cfg


def check_describe(row, cfg, case, host_only=False):
    for layout in row_layouts(row):
        if host_only and row.get("mp_combine"):      # (a host-only context does not read HRX_MP_COMBINE: ask the planner as a context created now would)
            os.environ["HRX_MP_COMBINE"] = "1"
            try:
                text = cfg.describe_launch(case.B, layout=layout, num_cus=255)
            finally:
                os.environ.pop("HRX_MP_COMBINE", None)
        else:
            text = cfg.describe_launch(case.B, layout=layout)
        assert re.search(row_expect(row, case.D, case.M), text), (row["id"], case.seed, layout, text)


def _cases(row):
    return [fd.make_case(s, row["shape"]) for s in fd.extra_seeds(row.get("seeds", SEEDS))]


def fr_case(row, cases):
    """the seed whose fr_columns the row checks: many strings, a real M (and one def where the row asks for the stripes form)"""
    for c in cases:
        if c.B >= 63 and c.M >= 16 and (row["fr"] != "D1" or c.D == 1):
            return c.seed
    return None


# ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hra():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    import halo2_regex_amd as m
    return m


def _guarded(torch, dev, nbytes, dtype):
    """a poisoned buffer of nbytes + GUARD bytes; returns (the caller's view of nbytes as dtype, the whole byte buffer)"""
    raw = torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device=dev)
    return raw[:nbytes].view(dtype), raw


def _guards_intact(raw, nbytes, what):
    tail = raw[nbytes:]
    bad = (tail != POISON).nonzero()
    assert bad.numel() == 0, "%s: a write %d bytes behind the buffer" % (what, int(bad[0]))


def _compare(row, case, ost, orec, omsk, st, rec, msk):
    """the first difference against the oracle, or None"""
    if not np.array_equal(st, ost):
        b = int(np.nonzero(st != ost)[0][0])
        return "status of string %d: got %#x want %#x" % (b, int(st[b]), int(ost[b]))
    ok = (ost & np.uint64(0xff)) == 0
    for name, got, want in (("records", rec, orec), ("masked", msk, omsk)):
        diff = (got != want)
        diff = diff.reshape(len(ok), -1).any(axis=1) & ok
        if diff.any():
            b = int(np.nonzero(diff)[0][0])
            where = np.argwhere(got[b] != want[b])[0]
            return "%s of string %d at %s: got %s want %s" % (name, b, tuple(int(x) for x in where), got[b][tuple(where)], want[b][tuple(where)])
    return None


def _stripe_sizes(hra, B, M, R):
    npl, nm = C.c_size_t(0), C.c_size_t(0)
    hra.lib.hrx_position_major_stripe_sizes(B, M, R, C.byref(npl), C.byref(nm))
    return npl.value, nm.value


def launch_every_form(hra, row, case, cfg, o, ost, tag, fr=False, pitched=None, alloc=None, stream=None):
    """The row's entry point on one case, every output into poisoned, guarded buffers (string-major: pitched ones on odd seeds, the pitch gaps checked; position-major:
    both input layouts, then record planes / row stripes); fr: fr_columns of the launch's rows as well.  Returns [(form, status, records (B, M, D), masked (B, M))].
    alloc(nbytes, dtype, kind) -> (view, raw): the caller's allocator for every buffer the library sees, the inputs included (raw: the bytes from the view's first on,
    GUARD poisoned ones behind it; tests/caller_conditions.py); stream: the launches go there, and it alone is waited for."""
    import torch
    dev = torch.device("cuda", 0)
    B, M, D, stride = case.B, case.M, case.D, case.stride
    d_chars = torch.from_numpy(case.chars).to(dev)
    d_lens = torch.from_numpy(case.lens.astype(np.int32)).to(dev)
    skw = {} if stream is None else dict(stream=stream)
    sync = torch.cuda.synchronize if stream is None else stream.synchronize
    if alloc is None:
        def _guarded_(nbytes, dtype, kind):
            return _guarded(torch, dev, nbytes, dtype)

        def to_pm(c):
            return hra.chars_to_position_major(c)
    else:
        _guarded_ = alloc

        def to_pm(c):
            v = alloc(c.numel(), torch.uint8, "chars_pm")[0]
            v.copy_(hra.chars_to_position_major(c))
            return v
        c_v, l_v = alloc(B * stride, torch.uint8, "chars")[0].view(B, stride), alloc(B * 4, torch.int32, "lens")[0]
        c_v.copy_(d_chars)
        l_v.copy_(d_lens)
        d_chars, d_lens = c_v, l_v
    runs = []      # (form, st, rec (B, M, D) numpy u32, msk (B, M) numpy u16)
    if row["entry"] == "sm":
        pitched = case.seed % 2 == 1 if pitched is None else pitched
        rp, mp = hra.recommended_pitches(M)[:2] if pitched else (M, M)
        r_v, r_raw = _guarded_(B * rp * D * 4, torch.int32, "records")
        m_v, m_raw = _guarded_(B * mp * 2, torch.int16, "masked")
        s_v, s_raw = _guarded_(B * 8, torch.int64, "status")
        out = (r_v.view(B, rp, D)[:, :M], m_v.view(B, mp)[:, :M], s_v)
        cfg.witness_batch(d_chars, d_lens, out=out, **skw)
        sync()
        for raw, n, what in ((r_raw, B * rp * D * 4, "records"), (m_raw, B * mp * 2, "masked"), (s_raw, B * 8, "status")):
            _guards_intact(raw, n, tag + " " + what)
        if pitched:      # rows M.. of every string's slot are never written
            assert (r_raw[:B * rp * D * 4].view(B, rp, D * 4)[:, M:] == POISON).all(), tag + ": a write into the records' pitch gap"
            assert (m_raw[:B * mp * 2].view(B, mp, 2)[:, M:] == POISON).all(), tag + ": a write into the masked rows' pitch gap"
        runs.append(("string-major" + (" pitched" if pitched else ""), out[2].cpu().numpy().view(np.uint64),
                     out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy().view(np.uint16)))
        if fr:
            _check_fr(hra, torch, o, cfg, case, d_chars, d_lens, out, dict(position_major=False), ost, tag, alloc, stream)
    else:
        nr, nm = C.c_size_t(0), C.c_size_t(0)
        hra.lib.hrx_position_major_sizes(B, M, D, C.byref(nr), C.byref(nm))
        for pm_input in (False, True):
            r_v, r_raw = _guarded_(nr.value * 4, torch.int32, "records")
            m_v, m_raw = _guarded_(nm.value * 2, torch.int16, "masked")
            s_v, s_raw = _guarded_(B * 8, torch.int64, "status")
            if pm_input:
                src, kw = to_pm(d_chars), dict(chars_pm_stride=stride)
            else:
                src, kw = d_chars, {}
            cfg.witness_batch_position_major(src, d_lens, out=(r_v, m_v, s_v), **kw, **skw)
            sync()
            form = "position-major" + (" (position-major input)" if pm_input else "")
            for raw, n, what in ((r_raw, nr.value * 4, "records"), (m_raw, nm.value * 2, "masked"), (s_raw, B * 8, "status")):
                _guards_intact(raw, n, "%s %s %s" % (tag, form, what))
            r1, m1 = hra.position_major_to_string_major(r_v, m_v, B, M, D)
            runs.append((form, s_v.cpu().numpy().view(np.uint64), r1.cpu().numpy().view(np.uint32), m1.cpu().numpy().view(np.uint16)))
            if fr and pm_input:
                _check_fr(hra, torch, o, cfg, case, src, d_lens, (r_v, m_v, s_v), dict(position_major=True, **kw), ost, tag, alloc, stream)
        # record planes (D >= 2) or the two row stripes of one def.  Only the guards behind the buffers are checked: rows >= M of the last quad /
        # octet, and with it the second stripe's slot past the last quad, are unspecified by the layout (include/hrx.h) (the kernels may store whole quads)
        R = 2 if D == 1 else 1
        npl, nmp = _stripe_sizes(hra, B, M, R)
        planes, raws = [], []
        for _ in range(D * R):
            p_v, p_raw = _guarded_(npl * 4, torch.int32, "plane")
            planes.append(p_v)
            raws.append(p_raw)
        m_v, m_raw = _guarded_(nmp * 2, torch.int16, "masked")
        s_v, s_raw = _guarded_(B * 8, torch.int64, "status")
        pm_input = case.seed % 2 == 0
        src, kw = (to_pm(d_chars), dict(chars_pm_stride=stride)) if pm_input else (d_chars, {})
        form = "row stripes" if D == 1 else "record planes"
        if row.get("planes") is False:      # a multi-pass config has no one-launch planes path: the library refuses, it writes nothing
            with pytest.raises(hra.HrxError, match="record planes"):
                cfg.witness_batch_planes(src, d_lens, out=(planes, m_v, s_v), **kw, **skw)
            sync()
            for k, raw in enumerate(raws + [m_raw, s_raw]):
                assert (raw == POISON).all(), "%s %s %d: written by a refused call" % (tag, form, k)
            runs_planes = False
        else:
            cfg.witness_batch_planes(src, d_lens, out=(planes, m_v, s_v), **kw, **skw)
            sync()
            runs_planes = True
        for k, raw in enumerate(raws):
            _guards_intact(raw, npl * 4, "%s %s %d" % (tag, form, k))
        _guards_intact(m_raw, nmp * 2, tag + " " + form + " masked")
        _guards_intact(s_raw, B * 8, tag + " " + form + " status")
        if runs_planes:
            r1, m1 = hra.planes_to_string_major(planes, m_v, B, M, D)
            runs.append((form, s_v.cpu().numpy().view(np.uint64), r1.cpu().numpy().view(np.uint32), m1.cpu().numpy().view(np.uint16)))
        if runs_planes and fr:
            _check_fr(hra, torch, o, cfg, case, src, d_lens, (planes, m_v, s_v), dict(position_major=True, **kw), ost, tag + " " + form, alloc, stream)
    return runs


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_variant_on_edge_case_definitions(hra, oracle, row):
    import torch
    dev = torch.device("cuda", 0)
    codes, accepted, masked_nonzero, live = set(), False, False, False
    cases = _cases(row)
    fr_seed = fr_case(row, cases) if row.get("fr") else None
    assert fr_seed is not None or not row.get("fr"), row["id"]
    for case in cases:
        B, M, D, stride = case.B, case.M, case.D, case.stride
        cfg = make_config(hra, row, case, 0)
        check_describe(row, cfg, case)
        o = OracleDefs(oracle, [(a, subs) for a, subs, _ in case.defs_t])
        orec, omsk, ost = o.witness_batch(case.chars, case.lens, M, threads=min(16, os.cpu_count() or 1))
        code = (ost & np.uint64(0xff)).astype(np.int64)
        codes |= set(code.tolist())
        if B > 1:
            assert (code == 0).mean() >= 1 / 3, (row["id"], case.seed, np.bincount(code))
        accepted |= bool(((ost >> np.uint64(8)) & np.uint64(0xffffffff))[code == 0].any())
        masked_nonzero |= bool(omsk[code == 0].any())
        tag = "%s seed %d (B=%d M=%d D=%d)" % (row["id"], case.seed, B, M, D)
        runs = launch_every_form(hra, row, case, cfg, o, ost, tag, fr=case.seed == fr_seed)
        for form, st, rec, msk in runs:
            err = _compare(row, case, ost, orec, omsk, st, rec, msk)
            assert err is None, "%s, %s: %s" % (tag, form, err)
        # the comparison is live: one flipped bit of one status-0 string's record is reported
        if not live and (code == 0).any():
            form, st, rec, msk = runs[0]
            b = int(np.nonzero(code == 0)[0][-1])
            rec = rec.copy()
            rec[b, M - 1, D - 1] ^= np.uint32(1 << (case.seed % 26))
            assert _compare(row, case, ost, orec, omsk, st, rec, msk) is not None
            live = True
    assert live
    # not vacuous: every status the row can produce, an accepted state, a nonzero masked row
    # (status 2 is two defs flagging one row: the oracle sums the start / end flags over the defs, and one def flags a row at most once, however many
    # substring definitions it has — tests/test_variants_cpu.py checks that no one-def case gives status 2)
    want = {0, 1, 3} | ({2} if row["shape"].d_hi >= 2 else set())
    assert want <= codes, (row["id"], sorted(codes))
    assert accepted and masked_nonzero, row["id"]


_LUTS = {}


def lib_fr_columns(hra, D):
    return hra.lib.hrx_fr_num_columns(D)


def _check_fr(hra, torch, o, cfg, case, src, d_lens, out, kw, ost, tag, alloc=None, stream=None):
    """fr_columns of the launch's rows against F::from of the oracle's integer columns (tests/test_fr.py's helper), status-0 strings
    (alloc, stream: as launch_every_form takes them; the cells come from the allocator then)"""
    from test_fr import _expected_cells, _mont
    if "m" not in _LUTS:
        _LUTS["m"] = np.array([[(_mont(v) >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in range(65536)], np.uint64)
    ok = np.nonzero((ost & np.uint64(0xff)) == 0)[0]
    if alloc is not None:
        kw = dict(kw, cells=alloc(lib_fr_columns(hra, case.D) * case.B * case.M * 32, torch.int64, "cells")[0])
    if stream is not None:
        kw = dict(kw, stream=stream)
    cells = cfg.fr_columns(src, d_lens, out, **kw)
    (torch.cuda if stream is None else stream).synchronize()
    cells = cells.view(-1, case.B, case.M, 4)
    got = cells.cpu().numpy().view(np.uint64)
    want = _expected_cells(o, case.chars, np.minimum(case.lens, case.M), case.M, case.D, _LUTS["m"])
    assert np.array_equal(got[:, ok], want[:, ok]), tag + ": fr_columns"
