"""The fused-wide match on the device (HRX_OPT_MATCH_FUSED_WIDE = 1: match_wide_kernel behind match_batch, match_batch_ragged and match_selected on configs of
four to eight defs).  Expectations are the oracle's (witness_batch -> rle_masked / status); every test also holds the option-0 call (via rows) on
the same inputs against the same expectation, so the two routes are compared entry by entry.  Every def count, tile-edge lengths at every byte offset, overlap
and accept bit 7 at eight defs, selections with lanes that walk several strings, truncation, a capture on a fresh context, extract and route behind it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fuzz_defs as fd
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import OracleDefs
from test_match_cpu import CFG_H4, rle_masked
from test_match_gpu import DEV, _cfg, _expect
from test_match_wide_cpu import FUZZ_SEEDS, OPT, fuzz_cfg
from test_ragged_gpu import _column, _padded
from test_select_gpu import P32, P64, SEL, check_oracle, guarded, np_out, read_back, run_selected, selected_mask, to_dev, untouched

pytestmark = pytest.mark.gpu
BAD_LENGTH = 3
RAG = hra.LAYOUT_INPUT_RAGGED


def pair(names, M):
    """the same config twice: the option at 1 (fused wide) and at 0 (via rows)"""
    on, off = _cfg(names, M), _cfg(names, M)
    on.set_option(OPT, 1)
    return on, off


def check_full(got, want, max_spans=16):
    st, cnt, sp = got
    ost, (ecnt, eruns) = want
    assert np.array_equal(st, ost)
    assert cnt.tolist() == ecnt
    dec = hra.decode_spans(cnt, sp) if max_spans else None
    if max_spans:
        bad = [b for b in range(len(ost)) if dec[b] != eruns[b][:max_spans]]
        assert not bad, bad[:5]


def all_forms(cfg, chars, lens, values, offsets, want, D, max_spans=16, fused=True):
    """string-major, ragged and both selected layouts (the identity selection) against the oracle"""
    B = len(lens)
    d_chars, d_lens, d_vals, d_offs = to_dev(chars), to_dev(lens.astype(np.uint32)), to_dev(values), to_dev(offsets)
    for layout in (0, RAG, SEL, SEL | RAG):
        text = cfg.describe_match(B, layout=layout)
        assert text.startswith("hrx::match_wide_kernel<%d, " % D if fused else "via rows"), text
    check_full(np_out(cfg.match_batch(d_chars, d_lens, max_spans=max_spans)), want, max_spans)
    check_full(np_out(cfg.match_batch_ragged(d_vals, d_offs, max_spans=max_spans)), want, max_spans)
    sel = np.arange(B, dtype=np.uint32)
    check_oracle(run_selected(cfg, d_chars, sel, B, max_spans=max_spans, lens=d_lens), want, sel, B, max_spans)
    check_oracle(run_selected(cfg, d_vals, sel, B, max_spans=max_spans, offsets=d_offs), want, sel, B, max_spans)


@pytest.mark.parametrize("D", [4, 5, 6, 7, 8])
def test_every_def_count(oracle, D):
    """fuzz_defs cases of exactly D defs (partial DFAs, undefined transitions at tile borders, lengths 0 .. M + 1, every byte value); every case is fused
    (tests/test_match_wide_cpu.py holds that on the CPU too)"""
    edges = set()
    for seed in FUZZ_SEEDS:
        case = fd.make_case(seed, fd.Shape(D, D, "small", "any"))
        edges |= case.edges
        o = OracleDefs(oracle, [(a.encode(), [t.encode() for t in subs]) for a, subs, _ in case.defs_t])
        _, omsk, ost = o.witness_batch(case.chars, case.lens, case.M)
        want = (ost, rle_masked(omsk, case.lens, ost))
        values, offsets = _column(_padded(case.chars, case.lens, case.M), np.minimum(case.lens, case.M + 1), lead=seed)
        for value in (1, 0):
            cfg = fuzz_cfg(case, value, device=0)
            all_forms(cfg, case.chars, case.lens, values, offsets, want, D, max_spans=8, fused=value == 1)
    assert any(e.startswith("undef_") for e in edges) and any(e.startswith("len_") for e in edges) and any(e.startswith("byte_") for e in edges)


@pytest.mark.parametrize("M", [200, 64])
def test_tile_edges_at_every_byte_offset(oracle, M):
    B = 130
    edge = [0, 1, 15, 16, 17, 63, 64, 65, M - 1, M, M + 1]
    chars, _ = synth.headers_planted(B, M + 1, seed=3, stride=-(-(M + 2) // 16) * 16)
    lens = np.array((edge * 12)[:B], np.uint32)
    lens = np.clip(lens.astype(np.int64), 0, M + 1).astype(np.uint32)
    chars = _padded(chars, lens, M)
    want = _expect(oracle, CFG_H4, chars, lens, M)
    assert int((want[0] & np.uint64(0xff) == BAD_LENGTH).sum()) == int((lens > M).sum()) > 0
    on, off = pair(CFG_H4, M)
    shifts = set()
    for lead in range(16):          # sh = (lead + the lengths before) % 16: over the 16 leads every string starts at every byte offset of a chunk
        values, offsets = _column(chars, lens, lead=lead)
        shifts |= {(b, int(o) % 16) for b, o in enumerate(offsets[:-1])}
        got = np_out(on.match_batch_ragged(to_dev(values), to_dev(offsets)))
        check_full(got, want)
    assert len(shifts) == 16 * B
    values, offsets = _column(chars, lens, lead=5)
    all_forms(on, chars, lens, values, offsets, want, 4)
    all_forms(off, chars, lens, values, offsets, want, 4, fused=False)


def test_overlap_and_accept_bit_seven_at_eight_defs(oracle):
    M, B = 208, 300
    chars, lens = synth.headers_planted(B, M - 1, seed=3, stride=M)
    lens = lens.astype(np.uint32)
    want = _expect(oracle, CFG_H4 * 2, chars, lens, M)
    assert int((want[0] & np.uint64(0xff) == 2).sum()) > 100         # the doubled defs flag the same rows: kStatusFlagOverlap with the oracle's row
    values, offsets = _column(chars, lens, lead=3)
    on, off = pair(CFG_H4 * 2, M)
    all_forms(on, chars, lens, values, offsets, want, 8)
    all_forms(off, chars, lens, values, offsets, want, 8, fused=False)
    # a clean eight-def fuzz case whose last def accepts somewhere
    for seed in range(40):
        case = fd.make_case(seed, fd.Shape(8, 8, "small", "any"))
        o = OracleDefs(oracle, [(a.encode(), [t.encode() for t in subs]) for a, subs, _ in case.defs_t])
        _, omsk, ost = o.witness_batch(case.chars, case.lens, case.M)
        if int((((ost & np.uint64(0xff)) == 0) & ((ost >> np.uint64(15)) & np.uint64(1) == 1)).sum()):
            break
    else:
        pytest.fail("no eight-def fuzz case sets accept bit 7")
    want = (ost, rle_masked(omsk, case.lens, ost))
    values, offsets = _column(_padded(case.chars, case.lens, case.M), np.minimum(case.lens, case.M + 1), lead=1)
    all_forms(fuzz_cfg(case, 1, device=0), case.chars, case.lens, values, offsets, want, 8, max_spans=8)


def test_selected_permutation_past_the_batch_and_lanes_that_walk_several_strings(oracle):
    M, B = 200, 600
    chars, lens = synth.headers_planted(B, M - 1, seed=4, stride=208)
    lens = lens.astype(np.uint32)
    lens[::17] = M + 1
    chars = _padded(chars, lens, M)
    want = _expect(oracle, CFG_H4, chars, lens, M)
    values, offsets = _column(chars, lens, lead=9)
    rng = np.random.default_rng(2)
    third = rng.permutation(B)[:B // 3].astype(np.uint32)
    sel = np.concatenate([third[:90], np.array([B, B + 7, 0xFFFFFFFF, 0x80000000], np.uint32), third[90:]])
    on, off = pair(CFG_H4, M)
    for cfg in (on, off):
        check_oracle(run_selected(cfg, to_dev(chars), sel, B, lens=to_dev(lens)), want, sel, B)          # (check_oracle: unselected entries keep their pre-fill)
        check_oracle(run_selected(cfg, to_dev(values), sel, B, offsets=to_dev(offsets)), want, sel, B)
    # n_sel several times the grid's lanes: short strings, M = 64; every string is one of 2048 bodies cut to one of 65 lengths, and the oracle walks each
    # distinct (body, length) once
    M2, B2 = 64, 40000
    base, _ = synth.regex1_planted(2048, 63, seed=2, stride=64)       # (the set's last def is regex1: these strings reveal runs within 64 bytes)
    pick = rng.integers(0, 2048, B2)
    lens2 = rng.integers(0, 65, B2).astype(np.uint32)
    chars2 = np.zeros((B2, 80), np.uint8)
    chars2[:, :64] = base[pick]
    chars2[np.arange(80)[None, :] >= lens2.astype(np.int64)[:, None]] = 0
    _, first, inverse = np.unique(pick.astype(np.int64) * 65 + lens2, return_index=True, return_inverse=True)
    ost, (ecnt, eruns) = _expect(oracle, CFG_H4, chars2[first], lens2[first], M2)
    want2 = (ost[inverse], ([ecnt[j] for j in inverse], [eruns[j] for j in inverse]))
    assert sum(want2[1][0]) > 1000
    on2, off2 = pair(CFG_H4, M2)
    d_chars, d_lens = to_dev(chars2), to_dev(lens2)
    sel2 = np.concatenate([np.arange(B2, dtype=np.uint32)[::-1]] * 4)        # 160000 positions: more than the 256 x 2 x 256 lanes of the largest grid
    assert on2.describe_match(len(sel2), layout=SEL).startswith("hrx::match_wide_kernel<4, 1, ")     # (past a wave per SIMD: the one-by-one sweep)
    assert on2.describe_match(B2, layout=0).startswith("hrx::match_wide_kernel<4, 4, ")
    check_oracle(run_selected(on2, d_chars, sel2, B2, max_spans=4, lens=d_lens), want2, sel2, B2, 4)
    check_full(np_out(on2.match_batch(d_chars, d_lens, max_spans=4)), want2, 4)
    check_full(np_out(off2.match_batch(d_chars, d_lens, max_spans=4)), want2, 4)


def test_max_spans_truncation_and_status_only(oracle):
    M, B = 208, 300
    chars, lens = synth.headers_planted(B, M - 1, seed=5, stride=M)
    lens = lens.astype(np.uint32)
    want = _expect(oracle, CFG_H4, chars, lens, M)
    assert max(want[1][0]) > 1
    values, offsets = _column(chars, lens, lead=2)
    on, off = pair(CFG_H4, M)
    for cfg in (on, off):
        check_full(np_out(cfg.match_batch_ragged(to_dev(values), to_dev(offsets), max_spans=1)), want, 1)
        check_full(np_out(cfg.match_batch(to_dev(chars), to_dev(lens), max_spans=1)), want, 1)
    # max_spans = 0 with span_counts NULL: status only
    st = torch.full((B,), P64, dtype=torch.int64, device=DEV)
    d_vals, d_offs = to_dev(values), to_dev(offsets)
    assert hra.lib.hrx_match_batch_device_ragged(on._need_ctx(), d_vals.data_ptr(), d_offs.data_ptr(), B, M, st.data_ptr(), None, None, 0,
                                                 torch.cuda.current_stream().cuda_stream) == hra.HRX_OK
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy().view(np.uint64), want[0])


def test_capture_on_a_fresh_context(oracle):
    M, B = 208, 300
    chars, lens = synth.headers_planted(B, M - 1, seed=3, stride=M)
    lens = lens.astype(np.uint32)
    want = _expect(oracle, CFG_H4, chars, lens, M)
    values, offsets = _column(chars, lens, lead=3)
    d_vals, d_offs = to_dev(values), to_dev(offsets)
    on, off = pair(CFG_H4, M)
    out, full = guarded(B)
    s = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):            # no call before this one
        on.match_batch_ragged(d_vals, d_offs, out=out, stream=s)
    for _ in range(2):
        for f, p in zip(full, (P64, P32, P64)):
            f.fill_(p)
        torch.cuda.synchronize()
        g.replay()
        check_full(read_back(out, full, B), want)
    # via rows before its first use: HRX_ERR_STATE inside a capture, nothing written
    out0, full0 = guarded(B)
    dummy = torch.zeros(16, device=DEV)
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=s):
        dummy.add_(1)
        with pytest.raises(hra.HrxError) as e:
            off.match_batch_ragged(d_vals, d_offs, out=out0, stream=s)
    assert e.value.code == hra.HRX_ERR_STATE
    assert untouched(read_back(out0, full0, B), np.zeros(B, bool))


def test_extract_and_route_behind_it():
    M, B = 208, 300
    chars, lens = synth.headers_planted(B, M - 1, seed=7, stride=M)
    values, offsets = _column(chars, lens.astype(np.uint32), lead=3)
    d_vals, d_offs = to_dev(values), to_dev(offsets)
    on, off = pair(CFG_H4, M)
    a, b = on.extract_batch_ragged(d_vals, d_offs, max_spans=8), off.extract_batch_ragged(d_vals, d_offs, max_spans=8)
    torch.cuda.synchronize()
    R, nbytes = int(b.totals[0]), int(b.totals[1])
    assert R > 100 and torch.equal(a.totals, b.totals) and torch.equal(a.run_offsets, b.run_offsets)
    assert torch.equal(a.runs[:R], b.runs[:R]) and torch.equal(a.byte_offsets[:R + 1], b.byte_offsets[:R + 1]) and torch.equal(a.values[:nbytes], b.values[:nbytes])
    st_a, st_b = on.match_batch_ragged(d_vals, d_offs)[0], off.match_batch_ragged(d_vals, d_offs)[0]
    ra, rb = on.route(st_a, offsets=d_offs, bounds=[64, 128, M]), off.route(st_b, offsets=d_offs, bounds=[64, 128, M])
    torch.cuda.synchronize()
    assert torch.equal(ra.order, rb.order) and torch.equal(ra.bucket_offsets, rb.bucket_offsets)
