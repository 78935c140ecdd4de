"""The reveal mask's carries over long event-free ranges, on every kernel: the lever batches of tests/carry_defs.py (ranges of hundreds to 131070 rows that an
event or the string's end confirms or takes back, opened at and resolved at every quad, octet, tile and chunk border) through every forced witness variant of
tests/test_variants_gpu.py, the chunked launch with forced and with the planner's own chunks, the match entry points (fused, via rows, ragged) and fr_columns.

Everywhere: describe_launch / describe_match names the kernel the test means; status words equal the oracle's on every string, records and masked rows bit for
bit on the status-0 ones; the witness outputs go into poisoned, guarded buffers (the fix-up is a store loop of data-dependent length).  What the batches hold is
checked without a device by tests/test_carry_cpu.py."""
import dataclasses
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import carry_defs as cd
import halo2_regex_amd as hra_mod
from oracle_lib import OracleDefs
from test_match_cpu import rle_masked
from test_match_gpu import VARIANTS, _check as check_match, _run as run_match
from test_ragged_gpu import _column, _run_ragged
from test_variants_gpu import NO_HOST, ROWS, ROW_IDS, _compare, check_describe, hra, launch_every_form, make_config, row_layouts      # noqa: F401  (hra: the fixture)

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
DEV = torch.device("cuda", 0)
CAP = 4                       # max_spans of the match tests: the over-cap scenario holds 2 + 3 * CAP runs before its range is taken back


def _oracle_rows(oracle, case):
    o = OracleDefs(oracle, [(a, subs) for a, subs, _ in case.defs_t])
    orec, omsk, ost = o.witness_batch(case.chars, case.lens, case.M, threads=THREADS)
    assert np.array_equal((ost & np.uint64(0xff)).astype(np.int64), case.want)      # (tests/test_carry_cpu.py says which strings are status 1 / 2)
    return o, orec, omsk, ost


def _witness(hra, oracle, row, case, fr=False, pitched=None, planes_describe=False):
    cfg = make_config(hra, row, case, 0)
    check_describe(row, cfg, case)
    if planes_describe and case.D >= 2:      # (one def's two row stripes are never walked in chunks: a chunk's first tile is not a stripe boundary)
        for lay in (1, 3):
            assert re.search(row["expect"], cfg.describe_launch(case.B, layout=lay | hra.LAYOUT_RECORD_PLANES))
    o, orec, omsk, ost = _oracle_rows(oracle, case)
    tag = "%s lever batch (B=%d M=%d D=%d)" % (row["id"], case.B, case.M, case.D)
    runs = launch_every_form(hra, row, case, cfg, o, ost, tag, fr=fr, pitched=pitched)
    assert len(runs) >= (1 if row["entry"] == "sm" else 2 if row.get("planes") is False else 3)
    for form, st, rec, msk in runs:
        err = _compare(row, case, ost, orec, omsk, st, rec, msk)
        assert err is None, "%s, %s: %s" % (tag, form, err)
    longest = {k: max([min(r, case.M) - a for b in range(case.B) if not case.want[b] for a, r, kk in case.ranges[b] if kk == k]) for k in ("confirmed", "taken_back")}
    assert min(longest.values()) >= max(cd.FORCED_CHUNK, case.M - 80), longest
    print("%s | %s | longest confirmed %d, longest taken back %d rows" % (tag, re.sub(r" grid=.*", "", cfg.describe_launch(case.B, layout=row_layouts(row)[0])), longest["confirmed"], longest["taken_back"]))
    return cfg, (o, orec, omsk, ost)


def _second_m(shape):
    """a row count off the tile grid (tile_is_exact's second clause, a partial last tile): odd where the row takes any M or odd ones alone, M % 16 == 8 where
    the row takes no other (carry_defs.row_ms)"""
    return cd.row_ms(dataclasses.replace(shape, min_batch=0))[1]


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_every_witness_variant_on_the_lever_batch(hra, oracle, row):
    """each row of the variant matrix at the fewest and the most defs it admits: 2048 rows and 1001 / 2000 (2047 and 1001 for rows of M % 8 != 0, 2040 and 1000
    for rows of M % 16 == 8; the first alone where the variant needs 16384 strings, 320 / 321 where it needs 65600 and more)"""
    sh = row["shape"]
    for M in cd.row_ms(sh):
        for D in sorted({sh.d_lo, sh.d_hi}):
            case = cd.scenario_batch(M, chunk=cd.FORCED_CHUNK, min_batch=sh.min_batch, **cd.row_form(sh, D))
            # (odd: pitched string-major buffers, string-major input to the planes launch; even: the other way.  Rows of odd M alone: 2047 pitched, 1001 and 321 not)
            case.seed = D + ((M >> 1 if sh.m == "odd8" else M) & 1)
            _witness(hra, oracle, row, case)


def test_string_major_rows_of_three_defs_on_the_lever_batch(hra, oracle):
    """String-major outputs of three defs come from the position-major kernel's own string-major form, which the variant matrix has no row for: its walker
    ends its tiles itself and takes ranges back at the string's pitch.  The 'three' form at 2048 rows (checked without a device by
    tests/test_carry_cpu.py::test_forms_are_what_they_claim[three]), into pitched buffers."""
    row = dict(id="sm-three-defs", entry="sm", flags=0, shape=None, expect=r"witness_pm_kernel<3, false, \w+, false, true, false>")
    case = cd.scenario_batch(cd.WITNESS_M, chunk=cd.FORCED_CHUNK, **cd.FORMS["three"])
    case.seed = 3
    _witness(hra, oracle, row, case)


def _chunk_row(expect, flags):
    return dict(id="chunked", entry="pm", flags=flags, shape=None, expect=re.escape(expect))


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("M", [2048, 8192])
def test_forced_chunks(hra, oracle, M, D):
    """chunks of 4 tiles (kDbgForceSpec): 8 and 32 per string, ranges inside one chunk, across two and across all of them; interleaved records from both input
    layouts, then record planes / row stripes"""
    case = cd.scenario_batch(M, chunk=cd.FORCED_CHUNK, D=D)
    case.seed = D + M // 8192
    _witness(hra, oracle, _chunk_row("chunked=%dx4 tiles" % (M // 256), 0x80), case, planes_describe=True)


@pytest.mark.parametrize("M,chunk,kind,D", [c + (D,) for c in cd.CHUNKED if c[2] != "forced" for D in (1, 2, 3)], ids=lambda v: str(v))
def test_the_planners_own_chunks(hra, oracle, M, chunk, kind, D):
    """8 x 16, 32 x 32 and 32 x 64 tiles per string: a carry through up to 32 chunk summaries, the repair of a 4096-row chunk (out of interleaved records and out of
    record planes of 2 and 3 defs).  Beyond 8192 rows D = 1 runs the lean batch tests/test_carry_cpu.py checks; D = 2, 3 its 96 strings with the longest ranges (the
    oracle's rows for 2^16 .. 2^17-row strings are what this file's time goes into)."""
    case = cd.scenario_batch(M, chunk=chunk, D=D, lean=M > 8192, limit=96 if M > 8192 and D > 1 else None)
    case.seed = D
    _witness(hra, oracle, _chunk_row("chunked=%s tiles" % kind, 0), case, planes_describe=True)


@pytest.mark.parametrize("D", [1, 3])
def test_every_chunk_a_repair_item_then_none(hra, oracle, D):
    """a batch in which every chunk of every string is a repair item (the first chunk's pending rows are taken back just behind its border, every later one inherits
    start_mask = 1): the repair list filled to its capacity, chunks x B; then a batch that needs no repair on the same context (a stale list or counter would repair
    what is right), then both again.  The item counts are those of carry_defs.repair_items, the stitch kernel's rule modelled on the oracle's columns."""
    M, B = cd.WITNESS_M, 256
    row = _chunk_row("chunked=8x4 tiles", 0x80)
    full, none = cd.all_repair_batch(M, B, D=D), cd.no_repair_batch(M, B, D=D)
    cfg = make_config(hra, row, full, 0)
    check_describe(row, cfg, full)
    for case, per_string in ((full, M // cd.FORCED_CHUNK), (none, 0), (full, None), (none, None)):
        assert case.B == B
        o, orec, omsk, ost = _oracle_rows(oracle, case)
        if per_string is not None:
            items = [len(cd.repair_items(*cd.columns(o, case.chars[b, :case.lens[b]], M)[1:], int(case.lens[b]), cd.FORCED_CHUNK)) for b in range(B)]
            assert items == [per_string] * B
        for form, st, rec, msk in launch_every_form(hra, row, case, cfg, o, ost, "all-repair D=%d" % D):
            err = _compare(row, case, ost, orec, omsk, st, rec, msk)
            assert err is None, (form, err)


def test_forced_chunks_replayed_from_a_graph(hra, oracle):
    """four captured chunked launches (scout, compose, walk, stitch, repair each) into four output sets, replayed three times: every set the bytes of an eager launch,
    which equal the oracle's"""
    M = cd.WITNESS_M
    case = cd.scenario_batch(M, chunk=cd.FORCED_CHUNK, D=2)
    row = _chunk_row("chunked=8x4 tiles", 0x80)
    cfg, (o, orec, omsk, ost) = _witness(hra, oracle, row, case)
    B = case.B
    d_chars, d_lens = torch.from_numpy(case.chars).to(DEV), torch.from_numpy(case.lens.astype(np.int32)).to(DEV)
    ref = cfg.alloc_outputs_position_major(B, DEV)
    for t in ref:
        t.fill_(-1)          # (rows of a string whose status is not 0 keep the fill on both sides)
    cfg.witness_batch_position_major(d_chars, d_lens, out=ref)
    outs = [cfg.alloc_outputs_position_major(B, DEV) for _ in range(4)]
    torch.cuda.synchronize()
    r1, m1 = hra.position_major_to_string_major(ref[0], ref[1], B, M, case.D)
    assert _compare(row, case, ost, orec, omsk, ref[2].cpu().numpy().view(np.uint64), r1.cpu().numpy().view(np.uint32), m1.cpu().numpy().view(np.uint16)) is None
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            for out in outs:
                cfg.witness_batch_position_major(d_chars, d_lens, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    for _ in range(3):
        for out in outs:
            for t in out:
                t.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for out in outs:
            assert all(torch.equal(x, y) for x, y in zip(out, ref))


def test_both_sides_of_a_position_major_block_border(hra, oracle):
    """65600 strings: long confirmed and taken-back ranges in strings 65535 and 65536 (the last of one block of the position-major buffers, the first of the next),
    witness rows and match runs"""
    case = cd.block_border_batch(320)
    row = [r for r in ROWS if r["id"] == "pm-narrow"][0]
    cfg, (o, orec, omsk, ost) = _witness(hra, oracle, row, case)
    planted = np.flatnonzero(np.array(case.names) == "planted")      # (the short filler strings reveal nothing: no runs)
    assert not np.delete(omsk, planted, axis=0).any()
    ecnt, eruns = [0] * case.B, [[] for _ in range(case.B)]
    for b, c, r in zip(planted, *rle_masked(omsk[planted], case.lens[planted], ost[planted])):
        ecnt[b], eruns[b] = c, r
    check_match(run_match(cfg, case.chars, case.lens, max_spans=CAP, pm=True), (ost, (ecnt, eruns)), CAP)


def _match_cfg(case, flags):
    os.environ["HRX_DEBUG_FLAGS"] = str(flags | NO_HOST)
    try:
        defs = [hra_mod.RegexDefs(hra_mod.AllstrRegexDef(a), [hra_mod.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
        return hra_mod.RegexVerifyConfig.configure(case.M, defs, device=0)
    finally:
        os.environ.pop("HRX_DEBUG_FLAGS", None)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_match_and_ragged_variants(oracle, D):
    """match_batch (fused kernels and via rows, both input layouts) and match_batch_ragged over the variants of tests/test_match_gpu.py, max_spans = 4: the
    over-cap scenario's run count goes to 2 + 12 and back to 3 when its range is taken back.  Status, counts, spans up to the count."""
    M = cd.WITNESS_M
    case = cd.scenario_batch(M, chunk=cd.FORCED_CHUNK, D=D, second=D == 1, cap=CAP)
    o, orec, omsk, ost = _oracle_rows(oracle, case)
    ecnt, eruns = rle_masked(omsk, case.lens, ost)
    assert max(ecnt) > CAP and any(0 < c <= CAP and "over_cap" in nm for c, nm in zip(ecnt, case.names))
    want = (ost, (ecnt, eruns))
    for name, flags, kernel in VARIANTS:
        cfg = _match_cfg(case, flags)
        desc, rdesc = cfg.describe_match(case.B), cfg.describe_match(case.B, layout=hra_mod.LAYOUT_INPUT_RAGGED)
        if kernel == "via rows":
            assert desc.startswith("via rows") and rdesc.startswith("via rows") and "ragged_slice_kernel" in rdesc, (name, desc, rdesc)
        elif kernel:
            assert desc.startswith("hrx::match_lane_kernel<%d, %s> " % (D, kernel)), (name, desc)
            assert rdesc.startswith("hrx::match_ragged_kernel<%d, %s> " % (D, kernel)), (name, rdesc)
        for pm in (False, True):
            check_match(run_match(cfg, case.chars, case.lens, max_spans=CAP, pm=pm), want, CAP)
        for lead in (0, 7):
            values, offsets = _column(case.chars, case.lens, lead)
            check_match(_run_ragged(cfg, values, offsets, CAP), want, CAP)


def test_match_via_rows_through_the_chunked_launch(oracle):
    """8192-row strings: the match goes via rows, and the rows come from the planner's chunked launch"""
    case = cd.scenario_batch(8192, chunk=1024, D=2, cap=CAP)
    o, orec, omsk, ost = _oracle_rows(oracle, case)
    want = (ost, rle_masked(omsk, case.lens, ost))
    cfg = _match_cfg(case, 0)
    desc = cfg.describe_match(case.B)
    assert desc.startswith("via rows") and "chunked=8x16 tiles" in desc, desc
    for pm in (False, True):
        check_match(run_match(cfg, case.chars, case.lens, max_spans=CAP, pm=pm), want, CAP)
    values, offsets = _column(case.chars, case.lens, 3)
    check_match(_run_ragged(cfg, values, offsets, CAP), want, CAP)


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("M,limit", [(cd.WITNESS_M, 48), (30016, 8)])
def test_field_cells_of_a_long_revealed_filler_range(hra, oracle, M, limit, D):
    """fr_columns of a lever batch (interleaved records; row stripes at D = 1, record planes at D = 2): 2045 and 30013 consecutive rows with masked_char != 0 and
    masked_substr_id == 0 (48 scenario strings of 2048 rows, 8 of 30016)"""
    case = cd.scenario_batch(M, chunk=cd.FORCED_CHUNK if M == cd.WITNESS_M else 0, D=D, limit=limit)
    case.seed = D
    row = dict([r for r in ROWS if r["id"] == "pm-narrow"][0], fr="any")
    _, (o, orec, omsk, ost) = _witness(hra, oracle, row, case, fr=True)
    ok = (ost & np.uint64(0xff)) == 0
    filler = ((omsk[ok] & 0xff) != 0) & ((omsk[ok] >> 8) == 0)
    assert filler.sum(axis=1).max() >= M - 4
