"""EXTRACT on the device (include/hrx.h: hrx_extract_spans_device behind extract_batch / extract_batch_ragged / extract_spans): the list column of revealed
bytes against the expectation of tests/test_extract_cpu.py (the oracle's masked rows, rle_masked, bytes sliced from the test's own copy, numpy cumsum) for
string-major, position-major and ragged input; every output and the workspace behind poisoned guards; short caps; two position-major blocks; batch sizes
around every workgroup and scan border; a captured graph of match + extract replayed on rewritten input; a via-rows def set; the host entry on a device
context.  Everything bit for bit."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import OracleDefs
from test_extract_cpu import GUARD, Batch, batch, check_capped, check_full, column, expect, short_caps
from test_match_cpu import CFG_1, CFG_H4, _defs, rle_masked
from test_match_gpu import _placed

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NO_HOST = 0x20000000          # kDbgNoHost
P64, P32, P8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A
FORMS = ["sm", "pm", "ragged"]


def dev_cfg(make_cfg):
    os.environ["HRX_DEBUG_FLAGS"] = str(NO_HOST)
    try:
        return make_cfg(device=0)
    finally:
        os.environ.pop("HRX_DEBUG_FLAGS", None)


def _inputs(bt, form, alloc=None):
    """the batch on the device in one of the three input forms: (args, kwargs) of extract_batch / extract_batch_ragged, input byte count
    (alloc: the caller's allocator, tests/test_match_gpu.py _placed)"""
    if form == "ragged":
        values, offsets = column(bt.chars, bt.lens, lead=3)          # strings at odd addresses
        return "ragged", (_placed(alloc, torch.from_numpy(values).to(DEV), "values"), _placed(alloc, torch.from_numpy(offsets.astype(np.int64)).to(DEV), "offsets")), {}, len(values)
    d_chars = _placed(alloc, torch.from_numpy(np.ascontiguousarray(bt.chars)).to(DEV), "chars")
    d_lens = _placed(alloc, torch.from_numpy(bt.lens.astype(np.int32)).to(DEV), "lens")
    if form == "pm":
        return "padded", (_placed(alloc, hra.chars_to_position_major(d_chars), "chars_pm"), d_lens), {"chars_pm_stride": bt.chars.shape[1]}, bt.chars.size
    return "padded", (d_chars, d_lens), {}, bt.chars.size


OUT_KINDS = ["status", "counts", "spans", "run_offsets", "runs", "byte_offsets", "bytes_out", "totals", "workspace"]      # (for an allocator by argument kind)


def guarded_out(B, K, runs_cap, values_cap, alloc=None):
    """the nine tensors of alloc_extract as slices of poisoned buffers with GUARD elements behind each -> (out, full buffers, sizes)
    (alloc(nbytes, dtype, kind) -> (view, raw): the caller's allocator, which poisons with the byte P8; GUARD elements of its guard stand in `full`)"""
    sizes = [B, B, B * K, B + 1, runs_cap, runs_cap + 1, values_cap, 4, hra.extract_workspace_bytes(B) // 8]
    dts = [torch.int64, torch.int32, torch.int64, torch.int64, torch.int64, torch.int64, torch.uint8, torch.int64, torch.int64]
    poison = {torch.int64: P64, torch.int32: P32, torch.uint8: P8}
    if alloc is not None:
        isz = {torch.int64: 8, torch.int32: 4, torch.uint8: 1}
        full = [alloc(n * isz[dt], dt, kind)[1][:(n + GUARD) * isz[dt]].view(dt) for n, dt, kind in zip(sizes, dts, OUT_KINDS)]
    else:
        full = [torch.full((n + GUARD,), poison[dt], dtype=dt, device=DEV) for n, dt in zip(sizes, dts)]
    out = [f[:n] for f, n in zip(full, sizes)]
    out[2] = out[2].view(B, K)
    return tuple(out), full, sizes


def run_device(cfg, bt, form, K, want, runs_cap=None, values_cap=None, require_accept=0, alloc=None, stream=None):
    """match + extract on the device into guarded outputs; checks the guards, status / counts against the oracle and the capacity rule against `want`
    (alloc: the caller's allocator for inputs and outputs; stream: the launches go there and it alone is waited for)"""
    kind, args, kw, in_bytes = _inputs(bt, form, alloc)
    if stream is not None:
        kw = dict(kw, stream=stream)
    B = len(bt.lens)
    runs_cap = B * K if runs_cap is None else runs_cap
    values_cap = in_bytes if values_cap is None else values_cap
    out, full, sizes = guarded_out(B, K, runs_cap, values_cap, alloc)
    fn = cfg.extract_batch_ragged if kind == "ragged" else cfg.extract_batch
    ex = fn(*args, max_spans=K, require_accept=require_accept, out=out, **kw)
    (torch.cuda if stream is None else stream).synchronize()
    for f, n, name in zip(full, sizes, "status counts spans run_offsets runs byte_offsets values totals workspace".split()):
        assert bool((f[n:] == {8: P64, 4: P32, 1: P8}[f.element_size()]).all()), (name, form)
    host = [f.cpu().numpy() for f in full]
    st, cnt = host[0][:B].view(np.uint64), host[1][:B].view(np.uint32)
    keep = bt.lens <= bt.M
    assert np.array_equal(st[keep], bt.ost[keep]) and cnt.tolist() == list(bt.ecnt)
    got = (host[3][:B + 1].view(np.uint64), host[4].view(np.uint64), host[5].view(np.uint64), host[6], host[7][:4].view(np.uint64))
    J = check_capped(got, want, runs_cap, values_cap)
    return ex, J


@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("name", ["lever256", "lever256_second", "lever1001"])
def test_lever_matrix(name, K):
    bt = batch(name)
    cfg = dev_cfg(bt.make_cfg)
    want = expect(bt, K)
    via_host = cfg.extract_batch_host(bt.chars, bt.lens, max_spans=K)          # the host entry on the same (device) context
    check_full(via_host, want)
    for form in FORMS:
        ex, J = run_device(cfg, bt, form, K, want)
        assert J == len(want[1])
        assert hra.extracted_lists(ex) == hra.extracted_lists(via_host)


def test_every_border_at_once():
    """more than 70001 strings (two position-major blocks, 1094 gather workgroups, 274 count workgroups: two rounds of the scan), exact caps, every output and
    the workspace behind guards"""
    bt = batch("lever_border")
    assert len(bt.lens) >= 70001
    cfg = dev_cfg(bt.make_cfg)
    want = expect(bt, 4)
    R, nb = int(want[4][0]), int(want[4][1])
    assert int(want[4][2]) > 0
    for form in FORMS:
        _, J = run_device(cfg, bt, form, 4, want, runs_cap=R, values_cap=nb)
        assert J == R


SCAN = hra.lib.hrx_extract_workspace_bytes          # (its step: one count workgroup per 256 strings, 256 of them per round of the scan workgroup)
SMALL_B = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 256 * 256 - 1, 256 * 256, 256 * 256 + 1]


@pytest.mark.parametrize("B", SMALL_B)
def test_small_batches(B):
    assert SCAN(256) == SCAN(1) and SCAN(257) == SCAN(256) + 24          # the workgroup size the borders above are chosen for
    big = batch("stress64_%d" % SMALL_B[-1])
    bt = big.prefix(B)
    cfg = dev_cfg(bt.make_cfg)
    want = expect(bt, 4)
    for form in FORMS:
        _, J = run_device(cfg, bt, form, 4, want)
        assert J == len(want[1])


@pytest.mark.parametrize("form", FORMS)
def test_short_caps(form):
    bt = batch("stress256")
    cfg = dev_cfg(bt.make_cfg)
    want = expect(bt, 4)
    seen = set()
    for runs_cap, values_cap in short_caps(want):
        seen.add(run_device(cfg, bt, form, 4, want, runs_cap=runs_cap, values_cap=values_cap)[1])
    assert len(seen) >= 5 and 0 in seen and len(want[1]) in seen


@pytest.mark.parametrize("mask", [1, 2, 3])
def test_require_accept(mask):
    bt = batch("stress256")
    cfg = dev_cfg(bt.make_cfg)
    want = expect(bt, 16, require_accept=mask)
    assert 0 < int(want[4][0]) < int(expect(bt, 16)[4][0])
    for form in FORMS:
        run_device(cfg, bt, form, 16, want, require_accept=mask)


def test_clipping_of_hand_made_span_words():
    """the arrays of tests/test_extract_cpu.py's clipping test through the kernels: equal to the host form (which that test pins to literal values)"""
    cfg = dev_cfg(batch("stress256").make_cfg)
    word = lambda start, length, sid=1: start | length << 28 | sid << 56
    stride = 32
    chars = np.arange(3 * stride, dtype=np.uint8).reshape(3, stride)
    status = np.array([1 << 8, 1 << 8, 1 << 8], np.uint64)
    counts = np.array([2, 1, 1], np.uint32)
    spans = np.array([[word(4, 3), word(30, 9, 2)], [word(40, 5), 0], [word(0, (1 << 28) - 1), 0]], np.uint64)
    values = np.arange(64, dtype=np.uint8)
    offsets = np.array([3, 13, 9, 15], np.uint64)
    rspans = np.array([[word(8, 5), word(2, 2, 3)], [word(0, 4), 0], [word(5, 100), 0]], np.uint64)
    to = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)
    for src, sp, kw in ((chars, spans, {}), (hra.chars_to_position_major(chars), spans, {"chars_pm_stride": stride}), (values, rspans, {"offsets": to(offsets)})):
        want = hra.extract_spans_host(chars if "offsets" not in kw else values, status, counts, sp, offsets=offsets if "offsets" in kw else None)
        out = cfg.alloc_extract(3, 2, 96)
        ex = cfg.extract_spans(to(src), to(status), to(counts), to(sp), out[3:], **kw)
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in ex]
        R, nb = int(want.totals[0]), int(want.totals[1])
        assert nb in (37, 5)
        assert np.array_equal(got[6].view(np.uint64), want.totals) and np.array_equal(got[2].view(np.uint64), want.run_offsets)
        assert np.array_equal(got[3].view(np.uint64)[:R], want.runs[:R]) and np.array_equal(got[4].view(np.uint64)[:R + 1], want.byte_offsets[:R + 1])
        assert np.array_equal(got[5][:nb], want.values[:nb])


def _oracle_batch(oracle, names, chars, lens, M):
    _, omsk, ost = OracleDefs.from_files(oracle, names).witness_batch(chars, lens, M, threads=16)
    ecnt, eruns = rle_masked(omsk, lens, ost)
    return Batch("inline", chars, lens, M, ost, ecnt, eruns, None)


def test_graph_capture_replays_on_rewritten_input(oracle):
    """match + extract captured together on one stream after one eager call; replayed on a rewritten ragged input of another length mix"""
    M, B, K = 1024, 4096, 8
    cfg = dev_cfg(lambda device: hra.RegexVerifyConfig.configure(M, _defs(CFG_1), device=device))
    c1, l1 = synth.regex1_planted(B, M - 1, seed=5, stride=M)
    c2, l2 = synth.reveal_stress(B, M, seed=8)
    rng = np.random.default_rng(3)
    l1 = np.minimum(l1, rng.integers(0, M + 1, B)).astype(np.uint32)
    l2 = np.minimum(l2, rng.integers(M // 2, M + 1, B)).astype(np.uint32)
    cols = [column(c1, l1, lead=3), column(c2, l2, lead=11)]
    cap = max(len(v) for v, _ in cols)
    d_vals = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    d_offs = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    d_vals[:len(cols[0][0])].copy_(torch.from_numpy(cols[0][0]))
    d_offs.copy_(torch.from_numpy(cols[0][1].astype(np.int64)))
    out = cfg.alloc_extract(B, K, cap)
    cfg.extract_batch_ragged(d_vals, d_offs, max_spans=K, out=out)            # (eager first: the launch's one-time setup happens outside the capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ex = cfg.extract_batch_ragged(d_vals, d_offs, max_spans=K, out=out, stream=s)
    for (chars, lens), (v, o) in zip(((c1, l1), (c2, l2)), cols):
        d_vals[:len(v)].copy_(torch.from_numpy(v))
        d_offs.copy_(torch.from_numpy(o.astype(np.int64)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        bt = _oracle_batch(oracle, CFG_1, chars, lens, M)
        got = hra.Extracted(*[t.cpu().numpy().view(dt) for t, dt in zip(ex, (np.uint64, np.uint32, np.uint64, np.uint64, np.uint64, np.uint8, np.uint64))])
        assert np.array_equal(got.status, bt.ost)
        check_full(got, expect(bt, K))


def test_a_via_rows_def_set(oracle):
    """four defs: the match goes via rows (the witness launch into context scratch); the extract launches run behind it and leave that scratch alone"""
    M, B, K = 1024, 2048, 16
    chars, lens = synth.headers_planted(B, M - 1, seed=3, stride=M)
    lens[::7] = (lens[::7] // 3).astype(lens.dtype)
    bt = _oracle_batch(oracle, CFG_H4, chars, lens, M)
    bt.make_cfg = lambda device: hra.RegexVerifyConfig.configure(M, _defs(CFG_H4), device=device)
    cfg = dev_cfg(bt.make_cfg)
    assert cfg.describe_match(B).startswith("via rows")
    want = expect(bt, K)
    assert int(want[4][0]) > B
    for form in FORMS + ["sm"]:               # (string-major once more: the scratch of the first three calls is still what the match expects)
        _, J = run_device(cfg, bt, form, K, want)
        assert J == len(want[1])


def test_host_entry_on_a_device_context():
    bt = batch("stress256")
    cfg = dev_cfg(bt.make_cfg)
    host_cfg = bt.make_cfg()
    values, offsets = column(bt.chars, bt.lens, lead=5)
    a = cfg.extract_batch_host_ragged(values, offsets, max_spans=4)
    b = host_cfg.extract_batch_host_ragged(values, offsets, max_spans=4)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    want = expect(bt, 4)
    check_full(a, want)
    ex = cfg.extract_batch_ragged(torch.from_numpy(values).to(DEV), torch.from_numpy(offsets.astype(np.int64)).to(DEV), max_spans=4)
    torch.cuda.synchronize()
    assert hra.extracted_lists(ex) == hra.extracted_lists(a)
    assert np.array_equal(ex.totals.cpu().numpy().view(np.uint64), a.totals)
