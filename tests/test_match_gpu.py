"""Match-only entry points on the device (include/hrx.h MATCH: hrx_match_batch_device, hrx_match_batch_host on a device context): status
bit for bit the witness path's, revealed runs = the run-length encoding of the oracle's masked column, through the fused kernel and
"via rows", string-major and position-major input, across two position-major blocks, inside a captured graph."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fuzz_defs as fd
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import OracleDefs
from test_match_cpu import CFG_1, CFG_23, CFG_A, CFG_H3, CFG_H4, _defs, rle_masked

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NO_HOST = 0x20000000          # kDbgNoHost


def _cfg(names, M, flags=0):
    os.environ["HRX_DEBUG_FLAGS"] = str(flags | NO_HOST)
    try:
        return hra.RegexVerifyConfig.configure(M, _defs(names), device=0)
    finally:
        os.environ.pop("HRX_DEBUG_FLAGS", None)


def _expect(oracle, names, chars, lens, M):
    _, omsk, ost = OracleDefs.from_files(oracle, names).witness_batch(chars, lens, M, threads=16)
    return ost, rle_masked(omsk, lens, ost)


def _placed(alloc, t, kind):
    """t copied into the caller's allocation of that kind (alloc(nbytes, dtype, kind) -> (view, raw), tests/caller_conditions.py); no allocator: t itself"""
    if alloc is None:
        return t
    v = alloc(t.numel() * t.element_size(), t.dtype, kind)[0].view(t.shape)
    v.copy_(t)
    return v


def _match_out(alloc, B, max_spans):
    """status, counts, spans out of the caller's allocator (None without one: match_batch makes its own)"""
    if alloc is None:
        return None
    return (alloc(B * 8, torch.int64, "status")[0], alloc(B * 4, torch.int32, "counts")[0], alloc(B * max_spans * 8, torch.int64, "spans")[0].view(B, max_spans))


def _run(cfg, chars, lens, max_spans=16, pm=False, alloc=None, stream=None):
    d_chars = _placed(alloc, torch.from_numpy(chars).to(DEV), "chars")
    d_lens = _placed(alloc, torch.from_numpy(lens.astype(np.int32)).to(DEV), "lens")
    okw = {} if alloc is None else dict(out=_match_out(alloc, len(lens), max_spans))
    if stream is not None:
        okw["stream"] = stream
    if pm:
        st, cnt, sp = cfg.match_batch(_placed(alloc, hra.chars_to_position_major(d_chars), "chars_pm"), d_lens, max_spans=max_spans, chars_pm_stride=chars.shape[1], **okw)
    else:
        st, cnt, sp = cfg.match_batch(d_chars, d_lens, max_spans=max_spans, **okw)
    (torch.cuda if stream is None else stream).synchronize()
    return st.cpu().numpy().view(np.uint64), cnt.cpu().numpy().view(np.uint32), sp.cpu().numpy().view(np.uint64)


def _check(got, want, max_spans=16):
    st, cnt, sp = got
    ost, (ecnt, eruns) = want
    assert np.array_equal(st, ost)
    assert cnt.tolist() == ecnt
    dec = hra.decode_spans(cnt, sp)
    bad = [b for b in range(len(ecnt)) if dec[b] != eruns[b][:max_spans]]
    assert not bad, bad[:5]


SHAPES = [("regex1", CFG_1, 65536, 1024, synth.regex1_planted), ("regex23", CFG_23, 16384, 2048, synth.regex23_planted),
          ("headers3", CFG_H3, 4096, 4096, synth.headers_planted), ("headers4", CFG_H4, 8192, 1024, synth.headers_planted)]


@pytest.mark.parametrize("name,names,B,M,gen", SHAPES, ids=[s[0] for s in SHAPES])
def test_fused_and_via_rows_equal_the_oracle(oracle, name, names, B, M, gen):
    chars, lens = gen(B, M - 1, seed=3, stride=M)
    lens[::7] = (lens[::7] // 3).astype(lens.dtype)      # ragged
    want = _expect(oracle, names, chars, lens, M)
    for flags, kind in ((0, None), (1 << 32, "via rows")):
        cfg = _cfg(names, M, flags)
        desc = cfg.describe_match(B)
        if kind:
            assert desc.startswith(kind)
        _check(_run(cfg, chars, lens), want)
        _check(_run(cfg, chars, lens, pm=True), want)


def test_two_position_major_blocks_guard_and_host_route(oracle):
    M, B, K = 1024, 70000, 4
    chars, lens = synth.reveal_stress(B, M, seed=9)
    want = _expect(oracle, CFG_A, chars, lens, M)
    for flags in (0, 1 << 32):
        cfg = _cfg(CFG_A, M, flags)
        for pm in (False, True):
            d_chars = torch.from_numpy(chars).to(DEV)
            d_lens = torch.from_numpy(lens.astype(np.int32)).to(DEV)
            inp = hra.chars_to_position_major(d_chars) if pm else d_chars
            guard = 0x5A5A5A5A5A5A5A5A
            st = torch.full((B + 64,), guard, dtype=torch.int64, device=DEV)
            cnt = torch.full((B + 128,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            sp = torch.full((B * K + 64,), guard, dtype=torch.int64, device=DEV)
            cfg.match_batch(inp, d_lens, max_spans=K, chars_pm_stride=M if pm else None, out=(st[:B], cnt[:B], sp[:B * K].view(B, K)))
            torch.cuda.synchronize()
            assert bool((st[B:] == guard).all()) and bool((cnt[B:] == 0x5A5A5A5A).all()) and bool((sp[B * K:] == guard).all())
            _check((st[:B].cpu().numpy().view(np.uint64), cnt[:B].cpu().numpy().view(np.uint32), sp[:B * K].view(B, K).cpu().numpy().view(np.uint64)), want, K)
    host_cfg = hra.RegexVerifyConfig.configure(M, _defs(CFG_A), device=hra.HRX_DEVICE_NONE)
    dev_cfg = _cfg(CFG_A, M)
    a = host_cfg.match_batch_host(chars[:8192], lens[:8192], max_spans=K)
    b = dev_cfg.match_batch_host(chars[:8192], lens[:8192], max_spans=K)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2]))
    assert hra.decode_spans(a[1], a[2]) == hra.decode_spans(b[1], b[2])


def test_graph_capture_replays_the_fused_launch(oracle):
    M, B = 1024, 8192
    chars, lens = synth.regex1_planted(B, M - 1, seed=5, stride=M)
    cfg = _cfg(CFG_1, M)
    assert cfg.describe_match(B).startswith("hrx::match_lane_kernel<1, false, false> ")
    d_chars, d_lens = torch.from_numpy(chars).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV)
    eager = [t.clone() for t in cfg.match_batch(d_chars, d_lens)]
    torch.cuda.synchronize()
    out = tuple(torch.zeros_like(t) for t in eager)
    s = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cfg.match_batch(d_chars, d_lens, out=out, stream=s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager[0], out[0]) and torch.equal(eager[1], out[1])       # status, counts
    assert hra.decode_spans(eager[1].cpu().numpy().view(np.uint32), eager[2].cpu().numpy().view(np.uint64)) == \
        hra.decode_spans(out[1].cpu().numpy().view(np.uint32), out[2].cpu().numpy().view(np.uint64))   # (slots past a count are unspecified)
    _check(tuple(t.cpu().numpy().view(dt) for t, dt in zip(out, (np.uint64, np.uint32, np.uint64))), _expect(oracle, CFG_1, chars, lens, M))


@pytest.mark.parametrize("seed", list(range(0, 12)))
def test_fuzz_defs_fused_vs_via_rows(oracle, seed):
    """1 .. 3 defs of tests/fuzz_defs.py through the fused kernel and via rows (which takes the witness planner's own variant)"""
    case = fd.make_case(seed, fd.Shape(1, 3, "small", "any", min_batch=256))
    o = OracleDefs(oracle, [(a.encode(), [t.encode() for t in subs]) for a, subs, _ in case.defs_t])
    _, omsk, ost = o.witness_batch(case.chars, case.lens, case.M)
    want = (ost, rle_masked(omsk, case.lens, ost))
    for flags in (0, 1 << 32):
        os.environ["HRX_DEBUG_FLAGS"] = str(flags | NO_HOST)
        try:
            defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
            cfg = hra.RegexVerifyConfig.configure(case.M, defs, device=0)
        finally:
            os.environ.pop("HRX_DEBUG_FLAGS", None)
        _check(_run(cfg, case.chars, case.lens, max_spans=8), want, 8)


# the variant matrix: each forced the way tests/test_variants_gpu.py forces the witness kernels (HRX_DEBUG_FLAGS), with the match kernel its describe
# string must name.  WIDE runs the narrow walk (the WIDE table only speeds up the witness's record assembly) and BYTE the HALF walk (the BYTE table's
# pair-hash tags serve the witness's finisher): csrc/hrx_kernel.hip plan_match_launch.
VARIANTS = [("default", 0, None), ("narrow", 0x80000, "false, false"), ("wide", 0x200000, "false, false"), ("half", 0x400000, "false, true"),
            ("byte", 0x2000, "false, true"), ("global", 0x40000, "true, false"), ("via_rows", 1 << 32, "via rows")]


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("seed", [0, 3, 6])
def test_variant_matrix(oracle, D, seed):
    case = fd.make_case(seed * 3 + D - 1, fd.Shape(D, D, "small", "any", min_batch=320))
    o = OracleDefs(oracle, [(a.encode(), [t.encode() for t in subs]) for a, subs, _ in case.defs_t])
    _, omsk, ost = o.witness_batch(case.chars, case.lens, case.M)
    want = (ost, rle_masked(omsk, case.lens, ost))
    for name, flags, kernel in VARIANTS:
        os.environ["HRX_DEBUG_FLAGS"] = str(flags | NO_HOST)
        try:
            defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
            cfg = hra.RegexVerifyConfig.configure(case.M, defs, device=0)
        finally:
            os.environ.pop("HRX_DEBUG_FLAGS", None)
        desc = cfg.describe_match(case.B)
        if kernel == "via rows" or (kernel and "chunked" in cfg.describe_launch(case.B, layout=hra.LAYOUT_POSITION_MAJOR)):
            assert desc.startswith("via rows"), (name, desc)
        elif kernel:
            assert desc.startswith("hrx::match_lane_kernel<%d, %s> " % (D, kernel)), (name, desc)
        for pm in (False, True):
            _check(_run(cfg, case.chars, case.lens, max_spans=8, pm=pm), want, 8)


def test_via_rows_in_several_slices(oracle):
    """strings whose witness rows fill the scratch several times over: slices of string-major input, and slices inside a block of position-major
    input (gathered string-major first)"""
    M, B = 32768, 4500
    chars, lens = synth.regex1_planted(B, M - 1, seed=4, stride=M)
    lens[::5] = (lens[::5] // 7).astype(lens.dtype)
    want = _expect(oracle, CFG_1, chars, lens, M)
    cfg = _cfg(CFG_1, M, 1 << 32)
    assert cfg.describe_match(B).startswith("via rows, 2 slice(s)")
    assert "pm_input_slice_kernel" in cfg.describe_match(B, layout=hra.LAYOUT_INPUT_POSITION_MAJOR)
    _check(_run(cfg, chars, lens), want)
    _check(_run(cfg, chars, lens, pm=True), want)
