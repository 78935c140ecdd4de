"""ROUTE on the device (include/hrx.h: hrx_route_device / hrx_gather_to_position_major_device behind route / gather_to_position_major): the partition against
the numpy expectation of tests/test_route_cpu.py (searchsorted + a stable argsort over the oracle's status words) at every count-workgroup and scan border;
the gathered staging against chars_to_position_major of the numpy-gathered, zero-padded strings, string-major and ragged sources, hand-made and routed
selections, more than one position-major block; screen -> route -> gather -> witness per bucket against the oracle at each bucket's own M; a captured graph
of match + route replayed on rewritten input; a via-rows def set; a host-only context.  Every output and the workspace behind poisoned guards; bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import OracleDefs
from test_extract_cpu import GUARD, batch, column
from test_extract_gpu import dev_cfg
from test_match_cpu import CFG_A, CFG_H4, _defs
from test_match_gpu import _placed
from test_route_cpu import EIGHT, check_invariants, expect_route, lengths_of
from test_route_cpu import test_device_forms_on_a_host_only_context as _host_only_context

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
P64, P32, P8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A
BAD = 0xFFFFFFFF
_CFGS = {}


def cfg_of(name):
    """one device context per batch name for the whole module (off the host walk, as tests/test_extract_gpu.py dev_cfg makes it)"""
    if name not in _CFGS:
        _CFGS[name] = dev_cfg(batch(name).make_cfg)
    return _CFGS[name]


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))).to(DEV)


def guarded(sizes, dts):
    poison = {torch.int64: P64, torch.int32: P32, torch.uint8: P8}
    full = [torch.full((n + GUARD,), poison[dt], dtype=dt, device=DEV) for n, dt in zip(sizes, dts)]
    return tuple(f[:n] for f, n in zip(full, sizes)), full


def guards_intact(full, sizes):
    return all(bool((f[n:] == {8: P64, 4: P32, 1: P8}[f.element_size()]).all()) for f, n in zip(full, sizes))


def route_device(cfg, status, kw, B, bounds, require_accept, stream=None, alloc=None):
    """route into guarded outputs and a guarded workspace -> (order uint32, bucket_offsets uint64) on the host
    (alloc(nbytes, dtype, kind) -> (view, raw): the caller's allocator for every argument, which checks its own guards; the stream alone is waited for then)"""
    sizes = [B, len(bounds) + 2, hra.route_workspace_bytes(B) // 8]
    if alloc is not None:
        out = tuple(alloc(n * sz, dt, kind)[0] for n, sz, dt, kind in zip(sizes, (4, 8, 8), (torch.int32, torch.int64, torch.int64), ("order", "bucket_offsets", "workspace")))
        r = cfg.route(None if status is None else _placed(alloc, to_dev(status), "status_in"), bounds=bounds, require_accept=require_accept, out=out, stream=stream,
                      **{k: _placed(alloc, to_dev(v), k) for k, v in kw.items()})
        (torch.cuda if stream is None else stream).synchronize()
        return r.order.cpu().numpy().view(np.uint32), r.bucket_offsets.cpu().numpy().view(np.uint64)
    out, full = guarded(sizes, [torch.int32, torch.int64, torch.int64])
    r = cfg.route(None if status is None else to_dev(status), bounds=bounds, require_accept=require_accept, out=out, stream=stream,
                  **{k: to_dev(v) for k, v in kw.items()})
    torch.cuda.synchronize()
    assert guards_intact(full, sizes)
    return r.order.cpu().numpy().view(np.uint32), r.bucket_offsets.cpu().numpy().view(np.uint64)


SMALL_B = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537]


@pytest.mark.parametrize("B", SMALL_B)
def test_route_borders(B):
    """one count workgroup per 256 strings, 256 of them per round of the scan workgroup: the sizes around each border (extract's workgroup size)"""
    assert hra.route_workspace_bytes(256) == hra.route_workspace_bytes(1) and hra.route_workspace_bytes(257) == hra.route_workspace_bytes(256) + 72
    bt = batch("stress64_%d" % SMALL_B[-1]).prefix(B)
    cfg = cfg_of("stress64_%d" % SMALL_B[-1])
    for form in ("lens", "offsets"):
        kw, n, valid = lengths_of(bt, form, lead=3)
        for bounds in ([16, 64], EIGHT + [66]):
            for ra in (0, 1):
                order, bo = route_device(cfg, bt.ost, kw, B, bounds, ra)
                want = expect_route(bt.ost, n, valid, bounds, ra)
                assert np.array_equal(bo, want[1]) and np.array_equal(order, want[0]), (B, form, bounds, ra)
                check_invariants(order, bo, B)
    if B == SMALL_B[-1]:          # no screening, and a decreasing pair of offsets in the second count workgroup
        kw, n, valid = lengths_of(bt, "offsets", lead=3)
        offsets = kw["offsets"].copy()
        offsets[301] = offsets[300] - np.uint64(1)
        n, valid = np.diff(offsets.astype(np.int64)), np.diff(offsets.astype(np.int64)) >= 0
        order, bo = route_device(cfg, None, {"offsets": offsets}, B, [16, 64], 0)
        want = expect_route(None, np.where(valid, n, 0), valid, [16, 64], 0)
        assert np.array_equal(bo, want[1]) and np.array_equal(order, want[0]) and 300 in order[int(bo[2]):]


# ---- gathered staging -------------------------------------------------------------------------------------------------------------------------------
def expect_gather(strings, sel, stride):
    """strings: per source string its bytes (numpy uint8) or None where it has no valid length / does not fit its slot -> (chars_pm flat, lens_out)"""
    sm = np.zeros((len(sel), stride), np.uint8)
    lens_out = np.full(len(sel), BAD, np.uint32)
    for k, s in enumerate(sel.tolist()):
        if s < len(strings) and strings[s] is not None and len(strings[s]) <= stride:
            sm[k, :len(strings[s])] = strings[s]
            lens_out[k] = len(strings[s])
    return (hra.chars_to_position_major(sm) if len(sel) else np.zeros(0, np.uint8)), lens_out


def gather_device(cfg, src, sel, stride, alloc=None, stream=None, **kw):
    """(alloc: the caller's allocator for the selection and the outputs — src and the lengths are the caller's tensors —, which checks its own guards; stream: the
    launch goes there and it alone is waited for)"""
    n_sel = len(sel)
    sizes = [n_sel * stride, n_sel]
    if alloc is not None:
        out = (alloc(sizes[0], torch.uint8, "chars_pm_out")[0], alloc(sizes[1] * 4, torch.int32, "lens_out")[0])
        pm, lo = cfg.gather_to_position_major(src, _placed(alloc, to_dev(sel), "sel"), stride, out=out, **({} if stream is None else dict(stream=stream)), **kw)
        (torch.cuda if stream is None else stream).synchronize()
        return pm.cpu().numpy(), lo.cpu().numpy().view(np.uint32)
    out, full = guarded(sizes, [torch.uint8, torch.int32])
    pm, lo = cfg.gather_to_position_major(src, to_dev(sel), stride, out=out, **kw)
    torch.cuda.synchronize()
    assert guards_intact(full, sizes)
    return pm.cpu().numpy(), lo.cpu().numpy().view(np.uint32)


def edge_batch(B=97, src_stride=80, stride=64):
    """string-major bytes with 0xAA past each string's end (as synth.ragged leaves it) and lengths 0, 1, 15, 16, 17, stride - 1, stride, stride + 1 and
    random ones; string 5 claims more than its slot holds"""
    rng = np.random.default_rng(4)
    lens = rng.integers(0, stride + 1, B).astype(np.uint32)
    lens[:8] = [0, 1, 15, 16, 17, stride - 1, stride, stride + 1]
    lens[20], lens[40] = stride + 1, src_stride
    chars = synth.ALPHABET98[rng.integers(0, 98, (B, src_stride))].astype(np.uint8)
    chars[np.arange(src_stride)[None, :] >= lens.astype(np.int64)[:, None]] = 0xAA
    return chars, lens


def hand_made_sel(n_sel, B):
    """descending with repeats, then B itself, 2^32 - 1 and B - 1 early on, so that every n_sel from 3 on holds the bad indices"""
    sel = np.array([B - 1 - (k // 2) % B for k in range(n_sel)], np.uint32)
    if n_sel >= 3:
        sel[1], sel[2] = B, BAD
    if n_sel >= 16:
        sel[3:13] = [7, 6, 5, 4, 3, 2, 1, 0, 20, 40]
    return sel


@pytest.mark.parametrize("n_sel", [0, 1, 63, 64, 65])
def test_gather_hand_made_selection(n_sel):
    cfg = cfg_of("stress256")
    chars, lens = edge_batch()
    B, src_stride = chars.shape
    sel = hand_made_sel(n_sel, B)
    d_chars, d_lens = to_dev(chars), to_dev(lens)
    for stride in (64, 96):                       # 96 > src_stride: a string may fit the output slot and still claim more than its source slot holds
        slens = lens.copy()
        if stride == 96:
            slens[5] = src_stride + 5
        strings = [chars[b, :slens[b]] if slens[b] <= src_stride else None for b in range(B)]
        pm, lo = gather_device(cfg, d_chars, sel, stride, lens=to_dev(slens))
        want = expect_gather(strings, sel, stride)
        assert np.array_equal(lo, want[1]) and np.array_equal(pm, want[0]), (n_sel, stride)
    # the same strings as a column at odd addresses, one pair of offsets decreasing
    values, offsets = column(chars, lens, lead=3)
    offsets = offsets.copy()
    offsets[31] = offsets[30] - np.uint64(2)
    strings = [values[int(offsets[b]):int(offsets[b + 1])] if offsets[b + 1] >= offsets[b] else None for b in range(B)]
    assert strings[30] is None and B - 1 not in (30, 31)
    pm, lo = gather_device(cfg, to_dev(values), sel, 64, offsets=to_dev(offsets))
    want = expect_gather(strings, sel, 64)
    assert np.array_equal(lo, want[1]) and np.array_equal(pm, want[0]), n_sel
    if n_sel >= 16:
        assert (want[1] == BAD).sum() >= 3 and set(want[1].tolist()) >= {0, 1, 15, 16, 17, 63, 64, BAD}


def test_gather_routed_selection_over_a_block_border():
    """stress64_70001, bounds [64], no accept bit required: every string is kept, n_sel = 70001 > HRX_PM_BLOCK, so the output has two position-major blocks"""
    bt = batch("stress64_70001")
    cfg = cfg_of("stress64_70001")
    B = len(bt.lens)
    kw, n, valid = lengths_of(bt, "lens")
    order, bo = route_device(cfg, bt.ost, kw, B, [64], 0)
    want = expect_route(bt.ost, n, valid, [64], 0)
    assert np.array_equal(order, want[0]) and np.array_equal(bo, want[1])
    n_sel = int(bo[1])
    assert n_sel > hra.PM_BLOCK
    sel = order[:n_sel]
    chars = bt.chars.copy()
    chars[np.arange(chars.shape[1])[None, :] >= n[:, None]] = 0xAA
    strings = [chars[b, :n[b]] for b in range(B)]
    want = expect_gather(strings, sel, 64)
    pm, lo = gather_device(cfg, to_dev(chars), sel, 64, lens=to_dev(bt.lens.astype(np.uint32)))
    assert np.array_equal(lo, want[1]) and np.array_equal(pm, want[0])
    values, offsets = column(bt.chars, bt.lens, lead=3)
    pm, lo = gather_device(cfg, to_dev(values), sel, 64, offsets=to_dev(offsets))
    assert np.array_equal(lo, want[1]) and np.array_equal(pm, want[0])


def test_no_selection_is_the_identity_selection():
    """hrx_ragged_to_position_major_device (the <ragged, no index> instantiation) = gather with sel = arange(B); tests/test_ragged_gpu.py judges the former"""
    cfg = cfg_of("stress256")
    bt = batch("stress256")
    B = len(bt.lens)
    values, offsets = column(bt.chars, bt.lens, lead=9)
    d_vals, d_offs = to_dev(values), to_dev(offsets)
    for stride in (256, 128):                     # 128: the longer strings do not fit
        pm0, l0 = cfg.ragged_to_position_major(d_vals, d_offs, stride=stride)
        pm1, l1 = cfg.gather_to_position_major(d_vals, to_dev(np.arange(B, dtype=np.uint32)), stride, offsets=d_offs)
        torch.cuda.synchronize()
        assert torch.equal(pm0, pm1) and torch.equal(l0, l1)
        assert stride == 256 or int((l0 == -1).sum()) > 0


# ---- screen -> route -> gather -> witness ---------------------------------------------------------------------------------------------------------------
def test_end_to_end_per_bucket_witness_against_the_oracle(oracle):
    bt = batch("stress256")
    cfg = cfg_of("stress256")
    B, bounds = len(bt.lens), [16, 64, 256]
    values, offsets = column(bt.chars, bt.lens, lead=3)
    d_vals, d_offs = to_dev(values), to_dev(offsets)
    st, _, _ = cfg.match_batch_ragged(d_vals, d_offs, max_spans=4)
    r = cfg.route(st, offsets=d_offs, bounds=bounds, require_accept=1)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy().view(np.uint64), bt.ost)
    order, bo = r.order.cpu().numpy().view(np.uint32), r.bucket_offsets.cpu().numpy().view(np.uint64)
    kw, n, valid = lengths_of(bt, "offsets", lead=3)
    want = expect_route(bt.ost, n, valid, bounds, 1)
    assert np.array_equal(order, want[0]) and np.array_equal(bo, want[1])
    sizes = np.diff(bo.astype(np.int64))
    assert int((sizes[:3] > 0).sum()) >= 2 and int(sizes[3]) > 0
    o = OracleDefs.from_files(oracle, CFG_A)
    for j, M in enumerate(bounds):
        n_sel = int(sizes[j])
        if n_sel == 0:
            continue
        lo_k, hi_k = int(bo[j]), int(bo[j + 1])
        idx = order[lo_k:hi_k].astype(np.int64)
        stride = -(-M // 16) * 16
        chars_pm, d_lens = cfg.gather_to_position_major(d_vals, r.order[lo_k:hi_k], stride, offsets=d_offs)
        with cfg.circuit_size(M):
            rec_pm, msk_pm, st_j = cfg.witness_batch_position_major(chars_pm, d_lens, chars_pm_stride=stride)
        torch.cuda.synchronize()
        assert cfg.max_chars_size == 256
        assert np.array_equal(d_lens.cpu().numpy().view(np.uint32), bt.lens[idx].astype(np.uint32))
        orec, omsk, ost = o.witness_batch(bt.chars[idx], bt.lens[idx], M, threads=16)       # the oracle at this bucket's M is the yardstick
        rec, msk = hra.position_major_to_string_major(rec_pm, msk_pm, n_sel, M, 2)
        ok = (ost & np.uint64(0xff)) == 0        # (rows are the witness's where the status code is 0, as tests/test_ragged_gpu.py compares them)
        assert np.array_equal(st_j.cpu().numpy().view(np.uint64), ost), j
        assert np.array_equal(rec.cpu().numpy().view(np.uint32)[ok], orec[ok]) and np.array_equal(msk.cpu().numpy().view(np.uint16)[ok], omsk[ok]), j
        assert ok.any()


def test_graph_capture_replays_on_rewritten_input(oracle):
    """match_batch + route captured together on one stream (a linear graph) after one eager call; replayed on the bytes and lengths of a second batch"""
    bt = batch("stress256")
    cfg = cfg_of("stress256")
    B, M, bounds = len(bt.lens), 256, [16, 64, 256]
    c2, l2 = synth.reveal_stress(B, M, seed=8)
    assert c2.shape == bt.chars.shape
    _, _, ost2 = OracleDefs.from_files(oracle, CFG_A).witness_batch(c2, l2, M, threads=16)
    d_chars, d_lens = to_dev(bt.chars), to_dev(bt.lens.astype(np.uint32))
    mout = (torch.zeros(B, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros((B, 4), dtype=torch.int64, device=DEV))
    sizes = [B, len(bounds) + 2, hra.route_workspace_bytes(B) // 8]
    rout, full = guarded(sizes, [torch.int32, torch.int64, torch.int64])

    def both(stream=None):
        st, _, _ = cfg.match_batch(d_chars, d_lens, max_spans=4, out=mout, stream=stream)
        return cfg.route(st, lens=d_lens, bounds=bounds, require_accept=1, out=rout, stream=stream)

    both()                                      # (eager first: the launch's one-time setup happens outside the capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r = both(s)
    for chars, lens, ost in ((bt.chars, bt.lens, bt.ost), (c2, l2, ost2)):
        d_chars.copy_(torch.from_numpy(np.ascontiguousarray(chars)))
        d_lens.copy_(torch.from_numpy(lens.astype(np.int32)))
        rout[0].fill_(P32)
        rout[1].fill_(P64)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = expect_route(ost, lens.astype(np.int64), np.ones(B, bool), bounds, 1)
        assert np.array_equal(mout[0].cpu().numpy().view(np.uint64), ost)
        assert np.array_equal(r.order.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(r.bucket_offsets.cpu().numpy().view(np.uint64), want[1])
        assert guards_intact(full, sizes)
    assert not np.array_equal(ost2, bt.ost)


def test_a_via_rows_def_set(oracle):
    """four defs: the match goes via rows (the witness launch into context scratch); route behind it accepts any context and leaves that scratch alone"""
    M, B = 1024, 2048
    chars, lens = synth.headers_planted(B, M - 1, seed=3, stride=M)
    lens[::7] = (lens[::7] // 3).astype(lens.dtype)
    lens[::11] = (lens[::11] // 20).astype(lens.dtype)
    _, _, ost = OracleDefs.from_files(oracle, CFG_H4).witness_batch(chars, lens, M, threads=16)
    cfg = dev_cfg(lambda device: hra.RegexVerifyConfig.configure(M, _defs(CFG_H4), device=device))
    assert cfg.describe_match(B).startswith("via rows")
    d_chars, d_lens = to_dev(chars), to_dev(lens.astype(np.uint32))
    bounds = [64, 256, 1024]
    sizes = {}
    for ra in (0, 1, 7, 8):
        st, _, _ = cfg.match_batch(d_chars, d_lens, max_spans=4)
        r = cfg.route(st, lens=d_lens, bounds=bounds, require_accept=ra)
        torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy().view(np.uint64), ost)
        want = expect_route(ost, lens.astype(np.int64), np.ones(B, bool), bounds, ra)
        assert np.array_equal(r.order.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(r.bucket_offsets.cpu().numpy().view(np.uint64), want[1])
        sizes[ra] = np.diff(want[1].astype(np.int64)).tolist()
    # what the oracle says about this batch: two buckets without the screen, a one-string bucket and rejects with def 0 required, nothing with def 3
    assert sizes[0] == [187, 0, 1861, 0] and sizes[1] == [1, 0, 1686, 361] and sizes[7] == [0, 0, 1671, 377] and sizes[8] == [0, 0, 0, 2048]


def test_device_forms_on_a_host_only_context():
    _host_only_context()
