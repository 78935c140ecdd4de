"""Selected match on the device (include/hrx.h SELECTED: hrx_match_selected_device behind match_selected): the fused selected kernel over ragged and
string-major sources, every table form, lanes that walk several strings, via rows in one and in several slices, a captured launch replayed on a
rewritten selection and input, the screen -> route -> selected screen cascade, and extract / route behind the call.  Expectations are the oracle's, or
(where said) the unselected call's on the same batch, which tests/test_match_gpu.py and tests/test_ragged_gpu.py pin to the oracle.  Outputs are indexed
by string: every entry outside the selection must keep its poison, and the guards around the arrays stay intact."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fuzz_defs as fd
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import OracleDefs
from test_match_cpu import CFG_1, CFG_23, CFG_H3, CFG_H4, rle_masked
from test_match_gpu import DEV, NO_HOST, _cfg, _expect
from test_ragged_gpu import _column, _lengths, _mixed_lengths, _padded

pytestmark = pytest.mark.gpu
BAD_LENGTH = 3
GUARD = 64
P64 = int(np.array([0xDEADBEEFCAFEF00D], np.uint64).view(np.int64)[0])
P32 = int(np.array([0xABABABAB], np.uint32).view(np.int32)[0])
SEL = 16        # hra.LAYOUT_INPUT_SELECTED
FUSED = [(CFG_1, synth.regex1_planted), (CFG_23, synth.regex23_planted), (CFG_H3, synth.headers_planted)]
_CACHE = {}


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))).to(DEV)


def guarded(B, max_spans=16):
    """status / counts / spans of B strings, poisoned, with GUARD poisoned entries in front of and behind each -> (views, whole tensors)"""
    full = (torch.full((B + 2 * GUARD,), P64, dtype=torch.int64, device=DEV), torch.full((B + 2 * GUARD,), P32, dtype=torch.int32, device=DEV),
            torch.full((B + 2 * GUARD, max_spans), P64, dtype=torch.int64, device=DEV))
    return tuple(f[GUARD:GUARD + B] for f in full), full


def read_back(out, full, B):
    torch.cuda.synchronize()
    for f, p in zip(full, (P64, P32, P64)):
        assert bool((f[:GUARD] == p).all()) and bool((f[GUARD + B:] == p).all()), "guard overwritten"
    return tuple(t.cpu().numpy().view(dt) for t, dt in zip(out, (np.uint64, np.uint32, np.uint64)))


def selected_mask(sel, B):
    mask = np.zeros(B, bool)
    mask[sel[sel < B]] = True
    return mask


def untouched(got, mask):
    st, cnt, sp = got
    return bool((st[~mask].view(np.int64) == P64).all() and (cnt[~mask].view(np.int32) == P32).all() and (sp[~mask].view(np.int64) == P64).all())


def check_oracle(got, want, sel, B, max_spans=16):
    """selected entries = the oracle's status, run count and runs; every other entry = the poison"""
    st, cnt, sp = got
    ost, (ecnt, eruns) = want
    mask = selected_mask(sel, B)
    idx = np.flatnonzero(mask)
    assert np.array_equal(st[mask], ost[mask])
    assert cnt[mask].tolist() == [ecnt[b] for b in idx]
    dec = hra.decode_spans(cnt[mask], sp[mask])
    bad = [int(b) for k, b in enumerate(idx) if dec[k] != eruns[b][:max_spans]]
    assert not bad, bad[:5]
    assert untouched(got, mask)


def check_same(got, full, sel, B):
    """selected entries = the unselected call's on the same batch; every other entry = the poison"""
    mask = selected_mask(sel, B)
    assert np.array_equal(got[0][mask], full[0][mask]) and np.array_equal(got[1][mask], full[1][mask])
    assert hra.decode_spans(got[1][mask], got[2][mask]) == hra.decode_spans(full[1][mask], full[2][mask])
    assert untouched(got, mask)


def np_out(ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().view(dt) for t, dt in zip(ts, (np.uint64, np.uint32, np.uint64)))


def selections(B, seed=1):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(B).astype(np.uint32)
    mixed = np.concatenate([perm[:B // 2], np.array([B, B + 7, 0xFFFFFFFF, 0x80000000], np.uint32), perm[B // 2:B // 2 + 40]])
    return {"identity": np.arange(B, dtype=np.uint32), "reversed": np.arange(B, dtype=np.uint32)[::-1].copy(), "permutation": perm,
            "every_third": np.arange(0, B, 3, dtype=np.uint32), "empty": np.zeros(0, np.uint32), "past_the_batch": mixed[rng.permutation(len(mixed))]}


def run_selected(cfg, src, sel, B, max_spans=16, alloc=None, stream=None, **kw):
    """alloc(nbytes, dtype, kind) -> (view, raw): the caller's allocator (tests/caller_conditions.py) for the selection and the outputs, which it poisons like guarded()
    (src and the lengths are the caller's tensors already); stream: the launch goes there and it alone is waited for"""
    if alloc is None:
        out, full = guarded(B, max_spans)
        cfg.match_selected(src, to_dev(sel), max_spans=max_spans, out=out, **kw)
        return read_back(out, full, B)
    out = (alloc(B * 8, torch.int64, "status")[0], alloc(B * 4, torch.int32, "counts")[0], alloc(B * max_spans * 8, torch.int64, "spans")[0].view(B, max_spans))
    d_sel = alloc(len(sel) * 4, torch.int32, "sel")[0]
    d_sel.copy_(to_dev(sel))
    cfg.match_selected(src, d_sel, max_spans=max_spans, out=out, **({} if stream is None else dict(stream=stream)), **kw)
    (torch.cuda if stream is None else stream).synchronize()
    return tuple(t.cpu().numpy().view(dt) for t, dt in zip(out, (np.uint64, np.uint32, np.uint64)))


def edge_case(oracle, D, B=1000, M=208):
    """B strings at the tile-edge lengths for the D-def fused set: padded chars, lens, the ragged column, the oracle's expectation (made once)"""
    if ("edge", D) not in _CACHE:
        names, gen = FUSED[D - 1]
        chars, _ = gen(B, M, seed=3, stride=-(-(M + 1) // 16) * 16)
        lens = _lengths("edge", B, M, np.random.default_rng(D))
        chars = _padded(chars, lens, M)
        _CACHE[("edge", D)] = (names, chars, lens, _column(chars, lens, lead=3), _expect(oracle, names, chars, lens, M))
    return _CACHE[("edge", D)]


@pytest.mark.parametrize("source", ["ragged", "string_major"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_fused_walk(oracle, D, source):
    B, M = 1000, 208
    names, chars, lens, (values, offsets), want = edge_case(oracle, D, B, M)
    assert int((want[0] & np.uint64(0xff) == BAD_LENGTH).sum()) == int((lens > M).sum()) > 0
    cfg = _cfg(names, M)
    if source == "ragged":
        src, kw, layout, sname = to_dev(values), {"offsets": to_dev(offsets)}, hra.LAYOUT_INPUT_RAGGED, "hrx::RaggedSrc"
    else:
        src, kw, layout, sname = to_dev(chars), {"lens": to_dev(lens)}, hra.LAYOUT_STRING_MAJOR, "hrx::PaddedSrc"
    sels = selections(B)
    cuts = [int(M * (j + 1) / 8) for j in range(8)]
    sels["routed_by_length"] = cfg.route(None, bounds=cuts, **kw).order.cpu().numpy().view(np.uint32)
    assert sorted(sels["routed_by_length"].tolist()) == list(range(B))
    for kind, sel in sels.items():
        if len(sel):
            assert cfg.describe_match(len(sel), layout=SEL | layout).startswith("hrx::match_selected_kernel<%d, false, false, %s> grid=persistent " % (D, sname))
        check_oracle(run_selected(cfg, src, sel, B, **kw), want, sel, B)


VARIANTS = [("narrow", 0x80000, "false, false"), ("half", 0x400000, "false, true"), ("global", 0x40000, "true, false")]


@pytest.mark.parametrize("D", [1, 2, 3])
def test_table_forms(oracle, D):
    case = fd.make_case(D - 1, fd.Shape(D, D, "small", "any", min_batch=320))
    o = OracleDefs(oracle, [(a.encode(), [t.encode() for t in subs]) for a, subs, _ in case.defs_t])
    M, B = case.M, case.B
    lens = case.lens.copy()
    lens[::11] = M + 1
    chars = _padded(case.chars, lens, M)
    _, omsk, ost = o.witness_batch(chars, lens, M)
    want = (ost, rle_masked(omsk, lens, ost))
    values, offsets = _column(chars, lens, lead=7)
    sel = np.random.default_rng(D).permutation(B).astype(np.uint32)
    for name, flags, kernel in VARIANTS:
        os.environ["HRX_DEBUG_FLAGS"] = str(flags | NO_HOST)
        try:
            defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
            cfg = hra.RegexVerifyConfig.configure(M, defs, device=0)
        finally:
            os.environ.pop("HRX_DEBUG_FLAGS", None)
        for src, kw, layout, sname in ((to_dev(values), {"offsets": to_dev(offsets)}, hra.LAYOUT_INPUT_RAGGED, "hrx::RaggedSrc"),
                                       (to_dev(chars), {"lens": to_dev(lens)}, hra.LAYOUT_STRING_MAJOR, "hrx::PaddedSrc")):
            desc = cfg.describe_match(B, layout=SEL | layout)
            if "chunked" in cfg.describe_launch(B, layout=hra.LAYOUT_POSITION_MAJOR):
                assert desc.startswith("via rows") and "selected_slice_kernel<%s>" % sname in desc, (name, desc)
            else:
                assert desc.startswith("hrx::match_selected_kernel<%d, %s, %s> " % (D, kernel, sname)), (name, desc)
            check_oracle(run_selected(cfg, src, sel, B, max_spans=8, **kw), want, sel, B, 8)


def test_a_lane_walks_more_than_one_string():
    """n_sel = 524288 + 300: a CU holds at most 2048 lanes and the device has 256 CUs, so the persistent grid has fewer lanes than strings.
    Equal to the unselected call on the same batch, both sources"""
    M, B = 64, 524288 + 300
    rng = np.random.default_rng(7)
    base, _ = synth.regex1_planted(4096, 32, seed=2, stride=48)
    lens = rng.integers(0, 33, B).astype(np.uint32)
    chars = np.zeros((B, 80), np.uint8)
    chars[:, :48] = base[rng.integers(0, 4096, B)]
    chars[np.arange(80)[None, :] >= lens.astype(np.int64)[:, None]] = 0
    values, offsets = _column(chars, lens, lead=5)
    sel = np.arange(B, dtype=np.uint32)[::-1].copy()
    cfg = _cfg(CFG_1, M)
    assert cfg.describe_match(B, layout=SEL | hra.LAYOUT_INPUT_RAGGED).startswith("hrx::match_selected_kernel<1, false, false, hrx::RaggedSrc> grid=persistent threads=256 ")
    d_vals, d_offs, d_chars, d_lens = to_dev(values), to_dev(offsets), to_dev(chars), to_dev(lens)
    full = np_out(cfg.match_batch_ragged(d_vals, d_offs, max_spans=4))
    assert int((full[1] > 0).sum()) > 1000
    check_same(run_selected(cfg, d_vals, sel, B, max_spans=4, offsets=d_offs), full, sel, B)
    check_same(run_selected(cfg, d_chars, sel, B, max_spans=4, lens=d_lens), full, sel, B)
    half = sel[::2].copy()
    check_same(run_selected(cfg, d_vals, half, B, max_spans=4, offsets=d_offs), full, half, B)


@pytest.mark.parametrize("names,flags", [(CFG_H4, 0), (CFG_1, 1 << 32)], ids=["headers4", "regex1_bit32"])
def test_via_rows(oracle, names, flags):
    B, M = 300, 208
    gen = synth.headers_planted if names is CFG_H4 else synth.regex1_planted
    chars, _ = gen(B, M, seed=3, stride=-(-(M + 1) // 16) * 16)
    lens = _lengths("edge", B, M, np.random.default_rng(11))
    chars = _padded(chars, lens, M)
    values, offsets = _column(chars, lens, lead=3)
    want = _expect(oracle, names, chars, lens, M)
    cfg = _cfg(names, M, flags)
    rng = np.random.default_rng(2)
    subset = rng.permutation(B)[:170].astype(np.uint32)
    subset = np.concatenate([subset[:90], np.array([B, 0xFFFFFFFF], np.uint32), subset[90:]])
    for src, kw, layout, sname in ((to_dev(values), {"offsets": to_dev(offsets)}, hra.LAYOUT_INPUT_RAGGED, "hrx::RaggedSrc"),
                                   (to_dev(chars), {"lens": to_dev(lens)}, hra.LAYOUT_STRING_MAJOR, "hrx::PaddedSrc")):
        desc = cfg.describe_match(len(subset), layout=SEL | layout)
        assert desc.startswith("via rows, 1 slice(s) of %d strings: hrx::selected_slice_kernel<%s> + " % (len(subset), sname)), desc
        assert desc.endswith(" + hrx::spans_from_masked_selected_kernel")
        check_oracle(run_selected(cfg, src, subset, B, **kw), want, subset, B)
        st_only, full = guarded(B, 1)            # status only: the scan still carries the status words to their strings
        cfg.match_selected(src, to_dev(subset), max_spans=0, out=st_only, **kw)
        got = read_back(st_only, full, B)
        mask = selected_mask(subset, B)
        assert np.array_equal(got[0][mask], want[0][mask]) and bool((got[0][~mask].view(np.int64) == P64).all())


def test_via_rows_in_several_slices():
    """4500 selected of 4600 strings of up to 32768 bytes: a slot costs 229380 bytes of the 768 MiB scratch as a ragged string does, so a slice is
    3510 slots and the call takes two.  Equal to the unselected via-rows call on the same batch"""
    M, B, n_sel = 32768, 4600, 4500
    chars, lens = synth.regex1_planted(B, M - 1, seed=4, stride=M)
    lens[::5] = (lens[::5] // 7).astype(lens.dtype)
    lens[::131] = M + 1
    cfg = _cfg(CFG_1, M, 1 << 32)
    assert cfg.describe_match(n_sel, layout=SEL | hra.LAYOUT_STRING_MAJOR).startswith("via rows, 2 slice(s) of 3510 strings: hrx::selected_slice_kernel<hrx::PaddedSrc> + ")
    d_chars, d_lens = to_dev(chars), to_dev(lens.astype(np.uint32))
    full = np_out(cfg.match_batch(d_chars, d_lens))
    sel = np.random.default_rng(3).permutation(B)[:n_sel].astype(np.uint32)
    check_same(run_selected(cfg, d_chars, sel, B, lens=d_lens), full, sel, B)


def test_capture_replays_on_a_rewritten_selection_and_input(oracle):
    M, B = 1024, 8192
    cfg = _cfg(CFG_1, M)
    c1, _ = synth.regex1_planted(B, M, seed=5, stride=1040)
    c2, _ = synth.ragged(B, M, seed=8)
    l1, l2 = _mixed_lengths(B, M, 3), _mixed_lengths(B, M, 4)
    c1, c2 = _padded(c1, l1, M), _padded(c2, l2, M)
    v1, o1 = _column(c1, l1, lead=3)
    v2, o2 = _column(c2, l2, lead=11)
    rng = np.random.default_rng(6)
    n_sel = 5000
    s1, s2 = rng.permutation(B)[:n_sel].astype(np.uint32), rng.permutation(B)[:n_sel].astype(np.uint32)
    d_vals = torch.zeros(max(len(v1), len(v2)), dtype=torch.uint8, device=DEV)
    d_offs = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    d_sel = torch.zeros(n_sel, dtype=torch.int32, device=DEV)
    d_vals[:len(v1)].copy_(torch.from_numpy(v1))
    d_offs.copy_(torch.from_numpy(o1))
    d_sel.copy_(to_dev(s1))
    out, full = guarded(B)
    cfg.match_selected(d_vals, d_sel, offsets=d_offs, out=out)            # (eager first: the launch's one-time setup happens outside the capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cfg.match_selected(d_vals, d_sel, offsets=d_offs, out=out, stream=s)
    for chars, lens, v, o, sel in ((c1, l1, v1, o1, s1), (c2, l2, v2, o2, s2)):
        d_vals[:len(v)].copy_(torch.from_numpy(v))
        d_offs.copy_(torch.from_numpy(o))
        d_sel.copy_(to_dev(sel))
        for f, p in zip(full, (P64, P32, P64)):
            f.fill_(p)
        torch.cuda.synchronize()
        g.replay()
        check_oracle(read_back(out, full, B), _expect(oracle, CFG_1, chars, lens, M), sel, B)


def test_via_rows_inside_a_capture_on_a_fresh_context():
    """the scratch of a via-rows call is allocated at first use, not inside a capture: HRX_ERR_STATE, nothing launched, nothing written"""
    M, B = 208, 300
    chars, lens = synth.headers_planted(B, M - 1, seed=3, stride=M)
    cfg = _cfg(CFG_H4, M)
    d_chars, d_lens, d_sel = to_dev(chars), to_dev(lens.astype(np.uint32)), to_dev(np.arange(0, B, 2, dtype=np.uint32))
    out, full = guarded(B)
    dummy = torch.zeros(16, device=DEV)
    s = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dummy.add_(1)
        with pytest.raises(hra.HrxError) as e:
            cfg.match_selected(d_chars, d_sel, lens=d_lens, out=out, stream=s)
    assert e.value.code == hra.HRX_ERR_STATE
    got = read_back(out, full, B)
    assert untouched(got, np.zeros(B, bool))
    # outside a capture the same call runs, and equals the unselected one
    sel = np.arange(0, B, 2, dtype=np.uint32)
    check_same(run_selected(cfg, d_chars, sel, B, lens=d_lens), np_out(cfg.match_batch(d_chars, d_lens)), sel, B)


def _cascade_batch(B=6000, M=1024):
    """headers with the regex1 literal planted in about a third of the strings (the four-def set's last def is regex1)"""
    chars, lens = synth.headers_planted(B, M - 40, seed=9, stride=M)
    hit = np.frombuffer(b"email was meant for @bob.", np.uint8)
    lens = lens.astype(np.uint32)
    for b in range(0, B, 3):
        n = int(lens[b])
        chars[b, n:n + len(hit)] = hit
        lens[b] = n + len(hit)
    return chars, lens


def test_cascade_cheap_screen_then_the_four_def_set_on_the_survivors():
    M = 1024
    chars, lens = _cascade_batch(M=M)
    B = len(lens)
    d_chars, d_lens = to_dev(chars), to_dev(lens)
    a, b4 = _cfg(CFG_1, M), _cfg(CFG_H4, M)
    st_a, _, _ = a.match_batch(d_chars, d_lens)
    r = a.route(st_a, lens=d_lens, bounds=[M], require_accept=1)
    kept = int(r.bucket_offsets.cpu()[1])
    assert 0 < kept < B
    d_sel = r.order[:kept]
    sel = d_sel.cpu().numpy().view(np.uint32)
    acc = np_out((st_a,))[0]
    assert set(sel.tolist()) == set(np.flatnonzero(((acc & np.uint64(0xff)) == 0) & ((acc >> np.uint64(8)) & np.uint64(1) == 1)).tolist())
    out, full = guarded(B)
    b4.match_selected(d_chars, d_sel, lens=d_lens, out=out)
    check_same(read_back(out, full, B), np_out(b4.match_batch(d_chars, d_lens)), sel, B)


def test_extract_and_route_run_behind_it_unchanged():
    """unselected entries pre-filled with kStatusBadLength and count 0: extract gives the runs of the full match restricted to the selection, and route
    routes exactly the selected, accepted strings"""
    M, max_spans = 1024, 8
    chars, lens = _cascade_batch(B=3000, M=M)
    B = len(lens)
    d_chars, d_lens = to_dev(chars), to_dev(lens)
    cfg = _cfg(CFG_1, M)
    sel = np.random.default_rng(5).permutation(B)[:1100].astype(np.uint32)
    mask = selected_mask(sel, B)
    st = torch.full((B,), BAD_LENGTH, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
    sp = torch.zeros((B, max_spans), dtype=torch.int64, device=DEV)
    cfg.match_selected(d_chars, to_dev(sel), lens=d_lens, max_spans=max_spans, out=(st, cnt, sp))
    fst, fcnt, fsp = cfg.match_batch(d_chars, d_lens, max_spans=max_spans)
    # the full match restricted to the selection, by hand
    d_mask = torch.from_numpy(mask).to(DEV)
    rst = torch.where(d_mask, fst, torch.full_like(fst, BAD_LENGTH))
    rcnt = torch.where(d_mask, fcnt, torch.zeros_like(fcnt))
    got = cfg.extract_spans(d_chars, st, cnt, sp, cfg.alloc_extract(B, max_spans, chars.size)[3:])
    ref = cfg.extract_spans(d_chars, rst, rcnt, fsp, cfg.alloc_extract(B, max_spans, chars.size)[3:])
    torch.cuda.synchronize()
    R, nbytes = int(ref.totals[0]), int(ref.totals[1])
    assert R > 100 and torch.equal(got.totals, ref.totals) and torch.equal(got.run_offsets, ref.run_offsets)
    assert torch.equal(got.runs[:R], ref.runs[:R]) and torch.equal(got.byte_offsets[:R + 1], ref.byte_offsets[:R + 1]) and torch.equal(got.values[:nbytes], ref.values[:nbytes])
    r = cfg.route(st, lens=d_lens, bounds=[M], require_accept=1)
    torch.cuda.synchronize()
    kept = int(r.bucket_offsets.cpu()[1])
    f = fst.cpu().numpy().view(np.uint64)
    accepted = ((f & np.uint64(0xff)) == 0) & ((f >> np.uint64(8)) & np.uint64(1) == 1)
    assert r.order[:kept].cpu().numpy().view(np.uint32).tolist() == np.flatnonzero(mask & accepted).tolist() and kept > 100


def test_host_entry_through_the_device(oracle):
    """hrx_match_selected_host on a device context: the selected strings packed chunk by chunk, matched by the ragged chunk path, copied out to their own
    indices.  max_spans = 16384 makes a chunk hold at most 511 strings, so 1000 strings (about 910 with a valid length) take two chunks"""
    B, M = 1000, 208
    names, chars, lens, (values, offsets), want = edge_case(oracle, 1, B, M)
    cfg = _cfg(names, M)
    p64, p32 = np.uint64(0xDEADBEEFCAFEF00D), np.uint32(0xABABABAB)
    for max_spans, sels in ((16, selections(B)), (16384, {"identity": np.arange(B, dtype=np.uint32)})):
        for kind, sel in sels.items():
            for src, kw in ((values, {"offsets": offsets.astype(np.uint64)}), (chars, {"lens": lens})):
                out = np.full(B, p64, np.uint64), np.full(B, p32, np.uint32), np.full((B, max_spans), p64, np.uint64)
                check_oracle(cfg.match_selected_host(src, sel, max_spans=max_spans, out=out, **kw), want, sel, B, max_spans)
