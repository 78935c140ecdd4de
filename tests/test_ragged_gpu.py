"""Ragged input on the device (include/hrx.h RAGGED): hrx_match_batch_device_ragged = hrx_match_batch_device on the padded copy = the oracle,
through the fused ragged kernel (every table form) and via rows, over length mixes, two position-major blocks, fuzzed defs, a captured graph
replayed on rewritten input, the host entry through the device in several chunks, and hrx_ragged_to_position_major_device feeding the witness."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fuzz_defs as fd
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import OracleDefs
from test_match_cpu import CFG_1, CFG_A, _defs, rle_masked
from test_match_gpu import DEV, NO_HOST, SHAPES, VARIANTS, _cfg, _check, _expect, _match_out, _placed, _run

pytestmark = pytest.mark.gpu
BAD_LENGTH = 3


def _lengths(kind, B, M, rng):
    if kind == "all_M":
        return np.full(B, M, np.uint32)
    if kind == "uniform":
        return rng.integers(0, M + 1, B).astype(np.uint32)
    if kind == "skewed":        # most strings short, a few at M
        lens = rng.integers(0, max(2, M // 16), B).astype(np.uint32)
        lens[rng.random(B) < 0.03] = M
        return lens
    edge = np.array([0, 1, 15, 16, 17, 63, 64, 65, M - 1, M, M + 1], np.int64)
    return np.clip(edge[rng.integers(0, len(edge), B)], 0, M + 1).astype(np.uint32)      # tile edges (M + 1: kStatusBadLength)


def _mixed_lengths(B, M, seed):
    rng = np.random.default_rng(seed)
    q = B // 4
    lens = np.concatenate([_lengths(k, n, M, rng) for k, n in (("all_M", q), ("uniform", q), ("skewed", q), ("edge", B - 3 * q))])
    return lens[rng.permutation(B)]


def _column(chars, lens, lead=0):
    """the strings chars[b, :lens[b]] back to back after `lead` bytes (odd offsets where lead or lengths are odd), 16-byte padded"""
    L = lens.astype(np.int64)
    offsets = np.zeros(len(L) + 1, np.int64)
    np.cumsum(L, out=offsets[1:])
    offsets += lead
    values = np.full(-(-int(offsets[-1]) // 16) * 16 + 16, 0xAA, np.uint8)
    mask = np.arange(chars.shape[1])[None, :] < L[:, None]
    values[lead:int(offsets[-1])] = chars[mask]
    return values, offsets


def _padded(chars, lens, M):
    """string-major copy wide enough for lens (<= M + 1), bytes past each length zero"""
    stride = -(-(M + 1) // 16) * 16
    out = np.zeros((len(lens), stride), np.uint8)
    w = min(stride, chars.shape[1])
    out[:, :w] = chars[:, :w]
    out[np.arange(stride)[None, :] >= lens.astype(np.int64)[:, None]] = 0
    return out


def _run_ragged(cfg, values, offsets, max_spans=16, alloc=None, stream=None):
    okw = {} if alloc is None else dict(out=_match_out(alloc, len(offsets) - 1, max_spans))
    if stream is not None:
        okw["stream"] = stream
    st, cnt, sp = cfg.match_batch_ragged(_placed(alloc, torch.from_numpy(values).to(DEV), "values"), _placed(alloc, torch.from_numpy(offsets).to(DEV), "offsets"),
                                         max_spans=max_spans, **okw)
    (torch.cuda if stream is None else stream).synchronize()
    return st.cpu().numpy().view(np.uint64), cnt.cpu().numpy().view(np.uint32), sp.cpu().numpy().view(np.uint64)


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert hra.decode_spans(a[1], a[2]) == hra.decode_spans(b[1], b[2])


def _triple(oracle, cfg, names, chars, lens, M, lead=0, want=None, o=None, max_spans=16):
    """device ragged == device padded == oracle"""
    chars = _padded(chars, lens, M)
    values, offsets = _column(chars, lens, lead)
    if want is None:
        if o is None:
            want = _expect(oracle, names, chars, lens, M)
        else:
            _, omsk, ost = o.witness_batch(chars, lens, M, threads=16)
            want = (ost, rle_masked(omsk, lens, ost))
    got = _run_ragged(cfg, values, offsets, max_spans)
    _check(got, want, max_spans)
    _same(got, _run(cfg, chars, lens, max_spans))
    return got


@pytest.mark.parametrize("name,names,B,M,gen", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes_and_length_mixes(oracle, name, names, B, M, gen):
    chars, _ = gen(B, M, seed=3, stride=-(-(M + 1) // 16) * 16)
    lens = _mixed_lengths(B, M, seed=B)
    cfg = _cfg(names, M)
    desc = cfg.describe_match(B, layout=hra.LAYOUT_INPUT_RAGGED)
    if len(names) > 3 or "chunked" in cfg.describe_launch(B, layout=hra.LAYOUT_POSITION_MAJOR):      # (the padded match goes via rows there too)
        assert desc.startswith("via rows") and "hrx::ragged_slice_kernel" in desc, desc
    else:
        assert desc.startswith("hrx::match_ragged_kernel<%d, " % len(names)), desc
    _triple(oracle, cfg, names, chars, lens, M, lead=3)


def test_via_rows_in_several_slices(oracle):
    """ragged strings whose witness rows and staged input fill the scratch more than once: a string costs 131072 (records) + 65536 (masked rows) +
    32768 (staged input) + 4 (its length) = 229380 bytes of the 768 MiB, so a slice is 3510 strings and 4500 strings take two (3510 + 990)"""
    M, B = 32768, 4500
    chars, _ = synth.regex1_planted(B, M, seed=4, stride=-(-(M + 1) // 16) * 16)
    lens = _mixed_lengths(B, M, seed=B)
    cfg = _cfg(CFG_1, M, 1 << 32)
    assert cfg.describe_match(B, layout=hra.LAYOUT_INPUT_RAGGED).startswith("via rows, 2 slice(s) of 3510 strings")
    _triple(oracle, cfg, CFG_1, chars, lens, M, lead=3)


def test_half_table_dfa(oracle):
    M, B = 1024, 16384
    a_txt, sub = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=40)
    os.environ["HRX_DEBUG_FLAGS"] = str(NO_HOST)
    try:
        cfg = hra.RegexVerifyConfig.configure(M, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub)])], device=0)
    finally:
        os.environ.pop("HRX_DEBUG_FLAGS", None)
    assert cfg.describe_match(B, layout=hra.LAYOUT_INPUT_RAGGED).startswith("hrx::match_ragged_kernel<1, false, true> ")
    chars, _ = synth.ragged(B, M, seed=6, alphabet=np.arange(256, dtype=np.uint8))
    lens = _mixed_lengths(B, M, seed=1)
    _triple(oracle, cfg, None, chars, lens, M, lead=5, o=OracleDefs(oracle, [(a_txt.encode(), [sub.encode()])]))


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("seed", [0, 3])
def test_variant_matrix(oracle, D, seed):
    case = fd.make_case(seed * 3 + D - 1, fd.Shape(D, D, "small", "any", min_batch=320))
    o = OracleDefs(oracle, [(a.encode(), [t.encode() for t in subs]) for a, subs, _ in case.defs_t])
    M = case.M
    lens = case.lens.copy()
    lens[::11] = M + 1
    chars = _padded(case.chars, lens, M)
    _, omsk, ost = o.witness_batch(chars, lens, M)
    want = (ost, rle_masked(omsk, lens, ost))
    for name, flags, kernel in VARIANTS:
        os.environ["HRX_DEBUG_FLAGS"] = str(flags | NO_HOST)
        try:
            defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
            cfg = hra.RegexVerifyConfig.configure(M, defs, device=0)
        finally:
            os.environ.pop("HRX_DEBUG_FLAGS", None)
        desc = cfg.describe_match(case.B, layout=hra.LAYOUT_INPUT_RAGGED)
        if kernel == "via rows" or (kernel and "chunked" in cfg.describe_launch(case.B, layout=hra.LAYOUT_POSITION_MAJOR)):
            assert desc.startswith("via rows") and "ragged_slice_kernel" in desc, (name, desc)
        elif kernel:
            assert desc.startswith("hrx::match_ragged_kernel<%d, %s> " % (D, kernel)), (name, desc)
        for lead in (0, 7):
            _triple(oracle, cfg, None, chars, lens, M, lead=lead, want=want, max_spans=8)


@pytest.mark.parametrize("seed", list(range(0, 6)))
def test_fuzz_defs(oracle, seed):
    case = fd.make_case(100 + seed, fd.Shape(1, 3, "small", "any", min_batch=256))
    o = OracleDefs(oracle, [(a.encode(), [t.encode() for t in subs]) for a, subs, _ in case.defs_t])
    os.environ["HRX_DEBUG_FLAGS"] = str(NO_HOST)
    try:
        defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
        cfg = hra.RegexVerifyConfig.configure(case.M, defs, device=0)
    finally:
        os.environ.pop("HRX_DEBUG_FLAGS", None)
    _triple(oracle, cfg, None, case.chars, case.lens, case.M, lead=seed, o=o, max_spans=8)


def test_two_position_major_blocks_and_staging_for_the_witness(oracle):
    """B = 65536 + 300: the match, and ragged_to_position_major feeding witness_batch_position_major / witness_batch_planes (rows, masked
    rows and status = the oracle's; strings longer than the stride: kStatusBadLength)"""
    M, B = 1024, 65536 + 300
    chars, _ = synth.reveal_stress(B, M, seed=12)
    lens = _mixed_lengths(B, M, seed=2)
    chars = _padded(chars, lens, M)
    orec, omsk, ost = OracleDefs.from_files(oracle, CFG_A).witness_batch(chars, lens, M, threads=16)
    cfg = _cfg(CFG_A, M)
    _triple(oracle, cfg, CFG_A, chars, lens, M, lead=1, want=(ost, rle_masked(omsk, lens, ost)))
    values, offsets = _column(chars, lens, lead=9)
    d_vals, d_offs = torch.from_numpy(values).to(DEV), torch.from_numpy(offsets).to(DEV)
    stride = -(-M // 16) * 16
    chars_pm, d_lens = cfg.ragged_to_position_major(d_vals, d_offs, stride=stride)
    torch.cuda.synchronize()
    want_lens = np.where(lens > stride, 0xFFFFFFFF, lens).astype(np.uint32)
    assert np.array_equal(d_lens.cpu().numpy().view(np.uint32), want_lens)
    keep = np.where(lens <= stride, lens, 0).astype(np.int64)
    staged = np.where(np.arange(stride)[None, :] < keep[:, None], chars[:, :stride], 0).astype(np.uint8)
    ref_pm = hra.chars_to_position_major(torch.from_numpy(staged).to(DEV))
    assert torch.equal(chars_pm, ref_pm)                                   # zero past n_b, nothing of a too-long string
    rec_pm, msk_pm, st = cfg.witness_batch_position_major(chars_pm, d_lens, chars_pm_stride=stride)
    torch.cuda.synchronize()
    rec, msk = hra.position_major_to_string_major(rec_pm, msk_pm, B, M, 2)
    ok = (ost & np.uint64(0xff)) == 0        # (rows are the witness's where the status code is 0, as tests/test_planes_gpu.py compares them)
    assert np.array_equal(st.cpu().numpy().view(np.uint64), ost)
    assert np.array_equal(rec.cpu().numpy().view(np.uint32)[ok], orec[ok]) and np.array_equal(msk.cpu().numpy().view(np.uint16)[ok], omsk[ok])
    planes, pmsk, pst = cfg.witness_batch_planes(chars_pm, d_lens, chars_pm_stride=stride)
    torch.cuda.synchronize()
    prec, pm = hra.planes_to_string_major(planes, pmsk, B, M, D=2)
    assert np.array_equal(pst.cpu().numpy().view(np.uint64), ost)
    assert np.array_equal(prec.cpu().numpy().view(np.uint32)[ok], orec[ok]) and np.array_equal(pm.cpu().numpy().view(np.uint16)[ok], omsk[ok])
    assert int((ost & np.uint64(0xff) == BAD_LENGTH).sum()) == int((lens > M).sum()) > 0
    # the staged buffer into the padded match: the same results as the ragged match
    st2, cnt2, sp2 = cfg.match_batch(chars_pm, d_lens, chars_pm_stride=stride)
    torch.cuda.synchronize()
    _check((st2.cpu().numpy().view(np.uint64), cnt2.cpu().numpy().view(np.uint32), sp2.cpu().numpy().view(np.uint64)), (ost, rle_masked(omsk, lens, ost)))


def test_graph_capture_replays_on_rewritten_input(oracle):
    M, B = 1024, 8192
    cfg = _cfg(CFG_1, M)
    assert cfg.describe_match(B, layout=hra.LAYOUT_INPUT_RAGGED).startswith("hrx::match_ragged_kernel<1, false, false> ")
    c1, _ = synth.regex1_planted(B, M, seed=5, stride=1040)
    c2, _ = synth.ragged(B, M, seed=8)
    l1, l2 = _mixed_lengths(B, M, 3), _mixed_lengths(B, M, 4)
    v1, o1 = _column(_padded(c1, l1, M), l1, lead=3)
    v2, o2 = _column(_padded(c2, l2, M), l2, lead=11)
    cap = max(len(v1), len(v2))
    d_vals = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    d_offs = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    d_vals[:len(v1)].copy_(torch.from_numpy(v1))
    d_offs.copy_(torch.from_numpy(o1))
    out = (torch.zeros(B, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros((B, 16), dtype=torch.int64, device=DEV))
    cfg.match_batch_ragged(d_vals, d_offs, out=out)            # (eager first: the launch's one-time setup happens outside the capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cfg.match_batch_ragged(d_vals, d_offs, out=out, stream=s)
    for chars, lens, v, o in ((c1, l1, v1, o1), (c2, l2, v2, o2)):
        d_vals[:len(v)].copy_(torch.from_numpy(v))
        d_offs.copy_(torch.from_numpy(o))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = tuple(t.cpu().numpy().view(dt) for t, dt in zip(out, (np.uint64, np.uint32, np.uint64)))
        p = _padded(chars, lens, M)
        _check(got, _expect(oracle, CFG_1, p, lens, M))


def test_host_entry_through_the_device_in_chunks():
    """more than 64 MiB of input: several chunks of whole strings, each one byte range + its offsets; = the host walk and the device entry"""
    M, B = 1024, 100000
    chars, _ = synth.regex1_planted(B, M, seed=9, stride=1040)
    lens = np.random.default_rng(9).integers(600, M + 2, B).astype(np.uint32)
    lens[::97] = 0
    values, offsets = _column(_padded(chars, lens, M), lens, lead=5)
    assert int(offsets[-1]) > (72 << 20)
    offsets[1000] = offsets[999] - 1 if offsets[999] > 0 else 0          # a decreasing pair: kStatusBadLength
    dev_cfg = _cfg(CFG_1, M)
    host_cfg = hra.RegexVerifyConfig.configure(M, _defs(CFG_1), device=hra.HRX_DEVICE_NONE)
    via_dev = dev_cfg.match_batch_host_ragged(values, offsets.astype(np.uint64), max_spans=4)
    assert int(via_dev[0][999]) == BAD_LENGTH
    _same(via_dev, _run_ragged(dev_cfg, values, offsets, max_spans=4))
    _same(via_dev, host_cfg.match_batch_host_ragged(values, offsets.astype(np.uint64), max_spans=4))
