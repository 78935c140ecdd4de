"""The device entry points under the three things a caller may do that no other GPU test does (helpers: tests/caller_conditions.py; what the cases hold is
asserted without a device by tests/test_caller_conditions_cpu.py):

  1. every pointer at exactly the alignment include/hrx.h asks for (16, 8 or 4 bytes and no more), every buffer between two poisoned guards — and every
     pointer shifted by half of that is refused with HRX_ERR_ARG, nothing written
  2. every launch on a fresh non-blocking side stream, behind a delay, over inputs that hold a decoy until copies on that stream replace it; and the host
     wait include/hrx.h promises when a context's scratch changes streams
  3. one context for a sequence of batches of 129, 1, 65, 320, 64, 129 and 0 strings, no synchronization in between

through the run helpers of the tests of each entry (launch_every_form and the others take the allocator and the stream), against OracleDefs.witness_batch
(rle_masked of its masked rows for the match paths), bit for bit.

Measured on the MI355X (test_the_delay_and_the_host_return_times prints the figures of every run): the delay the side-stream tests queue is calibrated per
run from one probe of torch.cuda._sleep to DELAY_MS = 25 ms and came out at 24.8 - 24.9 ms by the device's events (about 59.7 million cycles); the 84 warm
calls on the default stream returned to the host in 28 - 37 us (median; 124 us at most), the 84 calls behind the delay in 14 - 15 us (median; 107 us at
most): the race window stays open more than 200 times longer than the slowest call needs to return.  The whole file takes about 20 s."""
import ctypes as C
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import caller_conditions as cc
import halo2_regex_amd as hra_mod
from oracle_lib import OracleDefs
from test_extract_cpu import batch, column, expect
from test_extract_gpu import dev_cfg, run_device
from test_match_cpu import rle_masked
from test_match_gpu import _check as check_match, _placed, _run as run_match
from test_ragged_gpu import _column, _run_ragged
from test_route_cpu import expect_route, lengths_of
from test_route_gpu import expect_gather, gather_device, route_device
from test_select_gpu import run_selected, selected_mask
from test_variants_gpu import NO_HOST, _compare, check_describe, hra, launch_every_form, make_config      # noqa: F401  (hra: the fixture)

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
DEV = torch.device("cuda", 0)
DELAY_MS = 25.0
ROWS = cc.all_rows()
ROW_IDS = [r["id"] for r in ROWS]
_EXPECT = {}


def expected(oracle, key, case):
    """(OracleDefs, records, masked, status) of a case, computed once per module and never changed"""
    if key not in _EXPECT:
        o = OracleDefs(oracle, [(a, subs) for a, subs, _ in case.defs_t])
        orec, omsk, ost = o.witness_batch(case.chars, case.lens, case.M, threads=THREADS)
        for a in (orec, omsk, ost):
            a.setflags(write=False)
        _EXPECT[key] = (o, orec, omsk, ost)
    return _EXPECT[key]


@pytest.fixture(scope="module")
def delay():
    """(cycles for torch.cuda._sleep, the delay they make in ms by the device's events)"""
    assert torch.cuda.is_available(), "these tests need the GPU"
    cycles, ms = cc.calibrate_delay(torch, DELAY_MS)
    assert ms >= DELAY_MS / 4, "the calibrated delay is %.3f ms" % ms
    return cycles, ms


def _flip_is_reported(row, case, ost, orec, omsk, run):
    """one flipped bit of a status-0 string's last record is a difference"""
    form, st, rec, msk = run
    code = ost & np.uint64(0xff)
    if not (code == 0).any():
        return False
    b = int(np.nonzero(code == 0)[0][-1])
    rec = rec.copy()
    rec[b, case.M - 1, case.D - 1] ^= np.uint32(1 << (case.seed % 26))
    assert _compare(row, case, ost, orec, omsk, st, rec, msk) is not None
    return True


def _compare_runs(row, case, tag, want, runs):
    o, orec, omsk, ost = want
    for form, st, rec, msk in runs:
        err = _compare(row, case, ost, orec, omsk, st, rec, msk)
        assert err is None, "%s, %s: %s" % (tag, form, err)


# =====================================================================================================================================================
# 1. minimum alignment, guards on both sides
# =====================================================================================================================================================
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_witness_rows_at_minimum_alignment(hra, oracle, row):
    """every row of the variant matrix and the forced chunked launch through launch_every_form (string-major pitched and not; position-major from both input
    layouts; record planes / row stripes; fr_columns where the row checks it), chars / records / masked / planes / cells at 16 mod 32, status at 8 mod 16,
    lens at 4 mod 8, the position-major input written into such a view too"""
    live = False
    cases, fr_seed = cc.alignment_cases(row)
    assert any(c.B % 64 for c in cases) and (any(c.M % 8 for c in cases) or row["id"] == cc.CHUNK_ROW_ID or row["shape"].m in ("m16", "m8", "m8x")), row["id"]
    for case in cases:
        cfg = make_config(hra, row, case, 0)
        check_describe(row, cfg, case)
        want = expected(oracle, (row["id"], case.seed), case)
        tag = "%s seed %d (B=%d M=%d D=%d) at minimum alignment" % (row["id"], case.seed, case.B, case.M, case.D)
        alloc = cc.MinAlign(torch, DEV)
        pitched = None if len(cases) < 2 or row["entry"] != "sm" else case is cases[0]      # (one case pitched, one not, whatever the seeds' parity)
        runs = launch_every_form(hra, row, case, cfg, want[0], want[3], tag, fr=case.seed == fr_seed, pitched=pitched, alloc=alloc)
        alloc.check(tag)
        assert len(runs) >= (1 if row["entry"] == "sm" else 2 if row.get("planes") is False else 3)
        _compare_runs(row, case, tag, want, runs)
        live = live or _flip_is_reported(row, case, want[3], want[1], want[2], runs[0])
    assert live


def _match_cfg(case, flags):
    os.environ["HRX_DEBUG_FLAGS"] = str(flags | NO_HOST)
    try:
        defs = [hra_mod.RegexDefs(hra_mod.AllstrRegexDef(a), [hra_mod.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
        return hra_mod.RegexVerifyConfig.configure(case.M, defs, device=0)
    finally:
        os.environ.pop("HRX_DEBUG_FLAGS", None)


def _match_want(oracle, D):
    case = cc.match_case(D)
    o, orec, omsk, ost = expected(oracle, ("match", D), case)
    key = ("match-runs", D)
    if key not in _EXPECT:
        _EXPECT[key] = rle_masked(omsk, case.lens, ost)
    return case, (ost, _EXPECT[key])


def _describe_match(cfg, case, name):
    desc = cfg.describe_match(case.B)
    kernel = {"narrow": "false, false", "global": "true, false", "half": "false, true"}.get(name)
    if kernel is None or "chunked" in cfg.describe_launch(case.B, layout=hra_mod.LAYOUT_POSITION_MAJOR):
        assert desc.startswith("via rows"), (name, desc)
    else:
        assert desc.startswith("hrx::match_lane_kernel<%d, %s> " % (case.D, kernel)), (name, desc)


def _match_selection(B):
    """a permutation's first two thirds, with indices past the batch among them"""
    perm = np.random.default_rng(5).permutation(B).astype(np.uint32)
    return np.concatenate([perm[:B // 3], np.array([B, 0xFFFFFFFF], np.uint32), perm[B // 3:2 * B // 3]])


def _check_selected(got, want, sel, B, max_spans, poison):
    """selected entries = the oracle's; every other entry still the allocator's poison"""
    st, cnt, sp = got
    ost, (ecnt, eruns) = want
    mask = selected_mask(sel, B)
    idx = np.flatnonzero(mask)
    assert 0 < len(idx) < B
    assert np.array_equal(st[mask], ost[mask])
    assert cnt[mask].tolist() == [ecnt[b] for b in idx]
    dec = hra_mod.decode_spans(cnt[mask], sp[mask])
    bad = [int(b) for k, b in enumerate(idx) if dec[k] != eruns[b][:max_spans]]
    assert not bad, bad[:5]
    for a in (st, cnt, sp):
        assert (a[~mask].view(np.uint8) == poison).all(), "an entry outside the selection was written"


def _every_match_form(cfg, case, want, alloc_of, stream=None):
    """match_batch from both input layouts, match_batch_ragged, match_selected over both sources; alloc_of() -> a fresh allocator per call"""
    K, B = cc.MATCH_SPANS, case.B
    skw = {} if stream is None else dict(stream=stream)
    n = 0
    for pm in (False, True):
        alloc = alloc_of()
        check_match(run_match(cfg, case.chars, case.lens, max_spans=K, pm=pm, alloc=alloc, **skw), want, K)
        alloc.check("match_batch pm=%s" % pm)
        n += 1
    values, offsets = _column(case.chars, case.lens, 7)
    alloc = alloc_of()
    check_match(_run_ragged(cfg, values, offsets, K, alloc=alloc, **skw), want, K)
    alloc.check("match_batch_ragged")
    sel = _match_selection(B)
    for source in ("ragged", "string_major"):
        alloc = alloc_of()
        if source == "ragged":
            src, kw = _placed(alloc, torch.from_numpy(values).to(DEV), "values"), dict(offsets=_placed(alloc, torch.from_numpy(offsets).to(DEV), "offsets"))
        else:
            src = _placed(alloc, torch.from_numpy(case.chars).to(DEV), "chars")
            kw = dict(lens=_placed(alloc, torch.from_numpy(case.lens.astype(np.int32)).to(DEV), "lens"))
        got = run_selected(cfg, src, sel, B, max_spans=K, alloc=alloc, **skw, **kw)
        alloc.check("match_selected " + source)
        _check_selected(got, want, sel, B, K, alloc.poison)
    return n + 3


@pytest.mark.parametrize("name,flags", cc.MATCH_VARIANTS, ids=[v[0] for v in cc.MATCH_VARIANTS])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_match_ragged_and_selected_at_minimum_alignment(oracle, D, name, flags):
    """match_batch (fused: narrow table, table in L2, HALF table; via rows) from both input layouts, match_batch_ragged and match_selected over a ragged and a
    string-major source: chars / values at 16 mod 32, offsets / status / counts / spans at 8 mod 16, lens / sel at 4 mod 8"""
    case, want = _match_want(oracle, D)
    cfg = _match_cfg(case, flags)
    _describe_match(cfg, case, name)
    assert _every_match_form(cfg, case, want, lambda: cc.MinAlign(torch, DEV)) == 5
    # the comparison is live: one flipped bit of a status word is reported
    st = want[0].copy()
    st[case.B // 2] ^= np.uint64(1 << 9)
    with pytest.raises(AssertionError):
        check_match((st, np.array(want[1][0], np.uint32), np.zeros((case.B, cc.MATCH_SPANS), np.uint64)), want, cc.MATCH_SPANS)


STAGING_B = (1, 63, 65, 129)


def _staging_batch(B):
    bt = batch("stress256").prefix(B)
    return bt, dev_cfg(bt.make_cfg)


def _staging_calls(cfg, bt, alloc_of, stream=None):
    """ragged_to_position_major, gather_to_position_major (both sources), chars_to_position_major_device, route (both length forms), extract (three input
    forms): each into a fresh allocator's buffers, against the numpy expectations of the tests of each entry"""
    B, stride = bt.chars.shape
    skw = {} if stream is None else dict(stream=stream)
    values, offsets = column(bt.chars, bt.lens, lead=3)
    n = np.minimum(bt.lens.astype(np.int64), stride)
    strings = [bt.chars[b, :n[b]] for b in range(B)]
    ident = np.arange(B, dtype=np.uint32)
    # -- the ragged batch staged for the witness
    alloc = alloc_of()
    out = (alloc(B * stride, torch.uint8, "chars_pm_out")[0], alloc(B * 4, torch.int32, "lens_out")[0])
    pm, lo = cfg.ragged_to_position_major(_placed(alloc, torch.from_numpy(values).to(DEV), "values"),
                                          _placed(alloc, torch.from_numpy(offsets.astype(np.int64)).to(DEV), "offsets"), stride=stride, out=out, **skw)
    (torch.cuda if stream is None else stream).synchronize()
    alloc.check("ragged_to_position_major")
    wpm, wlo = expect_gather(strings, ident, stride)
    assert np.array_equal(lo.cpu().numpy().view(np.uint32), wlo) and np.array_equal(pm.cpu().numpy(), wpm), "ragged_to_position_major"
    # -- a selection gathered out of both sources
    sel = np.concatenate([ident[::-1][:max(1, 2 * B // 3)], np.array([B, 0xFFFFFFFF], np.uint32)])
    wpm, wlo = expect_gather(strings, sel, stride)
    for source in ("ragged", "string_major"):
        alloc = alloc_of()
        if source == "ragged":
            src, kw = _placed(alloc, torch.from_numpy(values).to(DEV), "values"), dict(offsets=_placed(alloc, torch.from_numpy(offsets.astype(np.int64)).to(DEV), "offsets"))
        else:
            src = _placed(alloc, torch.from_numpy(np.ascontiguousarray(bt.chars)).to(DEV), "chars")
            kw = dict(lens=_placed(alloc, torch.from_numpy(bt.lens.astype(np.int32)).to(DEV), "lens"))
        pm, lo = gather_device(cfg, src, sel, stride, alloc=alloc, **skw, **kw)
        alloc.check("gather_to_position_major " + source)
        assert np.array_equal(lo, wlo) and np.array_equal(pm, wpm), "gather_to_position_major " + source
    # -- the library's own transpose of a string-major batch
    alloc = alloc_of()
    out = alloc(B * stride, torch.uint8, "chars_pm_out")[0]
    got = cfg.chars_to_position_major_device(_placed(alloc, torch.from_numpy(np.ascontiguousarray(bt.chars)).to(DEV), "chars"), out=out, **skw)
    (torch.cuda if stream is None else stream).synchronize()
    alloc.check("chars_to_position_major_device")
    assert np.array_equal(got.cpu().numpy(), hra_mod.chars_to_position_major(np.ascontiguousarray(bt.chars))), "chars_to_position_major_device"
    # -- route
    for form in ("lens", "offsets"):
        kw, nn, valid = lengths_of(bt, form, lead=3)
        alloc = alloc_of()
        order, bo = route_device(cfg, bt.ost, kw, B, [16, 64, 256], 1, stream=stream, alloc=alloc)
        alloc.check("route " + form)
        w = expect_route(bt.ost, nn, valid, [16, 64, 256], 1)
        assert np.array_equal(bo, w[1]) and np.array_equal(order, w[0]), "route " + form
    # -- extract: the five outputs and the workspace (the match outputs in front of them)
    wex = expect(bt, 4)
    for form in ("sm", "pm", "ragged"):
        alloc = alloc_of(0x5A)          # (the poison tests/test_extract_cpu.py check_capped looks for)
        _, J = run_device(cfg, bt, form, 4, wex, alloc=alloc, stream=stream)
        alloc.check("extract " + form)
        assert J == len(wex[1])
    return 9


@pytest.mark.parametrize("B", STAGING_B)
def test_staging_route_and_extract_at_minimum_alignment(B):
    """values / chars / chars_pm at 16 mod 32, every u64 array and the workspaces at 8 mod 16, lens / sel / order / lens_out at 4 mod 8, extract's values at an
    odd address (include/hrx.h has no rule for them)"""
    bt, cfg = _staging_batch(B)
    assert _staging_calls(cfg, bt, lambda poison=cc.POISON: cc.MinAlign(torch, DEV, poison)) == 9


# ---- the refusal matrix -----------------------------------------------------------------------------------------------------------------------------
def _refusals(entry, make_args, pointers, alloc):
    """each pointer argument of a device entry shifted by half its minimum alignment, one at a time: HRX_ERR_ARG, every output still poison.
    make_args(shift) -> the argument tuple with {index: bytes} added to the pointers; pointers: {argument index: minimum alignment}"""
    fn = getattr(hra_mod.lib, entry)
    seen = 0
    for idx, a in pointers.items():
        rc = fn(*make_args({idx: a // 2}))
        assert rc == hra_mod.HRX_ERR_ARG, "%s: argument %d shifted by %d bytes: rc %d (%s)" % (entry, idx, a // 2, rc, hra_mod.lib.hrx_last_error())
        seen += 1
    torch.cuda.synchronize()
    assert alloc.all_poison(), entry + ": a refused call wrote into an output"
    return seen


def test_misaligned_pointers_are_refused_and_nothing_is_written(hra):
    """hrx_witness_batch_device_pitched / _layout / _planes, hrx_match_batch_device / _ragged, hrx_match_selected_device, hrx_ragged_to_position_major_device,
    hrx_gather_to_position_major_device, hrx_chars_to_position_major_device, hrx_route_device and hrx_extract_spans_device on a device context"""
    bt, cfg = _staging_batch(8)
    B, stride, M, D, K = 8, bt.chars.shape[1], bt.M, 2, 4
    assert cfg.num_defs == D
    alloc = cc.MinAlign(torch, DEV)
    values, offsets = column(bt.chars, bt.lens, lead=3)
    chars = _placed(alloc, torch.from_numpy(np.ascontiguousarray(bt.chars)).to(DEV), "chars")
    lens = _placed(alloc, torch.from_numpy(bt.lens.astype(np.int32)).to(DEV), "lens")
    vals = _placed(alloc, torch.from_numpy(values).to(DEV), "values")
    offs = _placed(alloc, torch.from_numpy(offsets.astype(np.int64)).to(DEV), "offsets")
    sel = _placed(alloc, torch.arange(B, dtype=torch.int32, device=DEV), "sel")
    st_in = _placed(alloc, torch.from_numpy(bt.ost.view(np.int64).copy()).to(DEV), "status_in")

    def out(nbytes, kind):
        return alloc(nbytes, torch.uint8, kind)[0].data_ptr()
    nr, nm = C.c_size_t(0), C.c_size_t(0)
    hra.lib.hrx_position_major_sizes(B, M, D, C.byref(nr), C.byref(nm))
    npl, nmp = C.c_size_t(0), C.c_size_t(0)
    hra.lib.hrx_position_major_stripe_sizes(B, M, 1, C.byref(npl), C.byref(nmp))
    rec, msk, st = out(max(nr.value, B * M * D) * 4, "records"), out(max(nm.value, nmp.value, B * M) * 2, "masked"), out(B * 8, "status")
    planes = [out(npl.value * 4, "plane") for _ in range(D)]
    cnt, sp = out(B * 4, "counts"), out(B * K * 8, "spans")
    pm_out, lens_out = out(B * stride, "chars_pm_out"), out(B * 4, "lens_out")
    order, bo, rws = out(B * 4, "order"), out(4 * 8, "bucket_offsets"), out(hra.route_workspace_bytes(B), "workspace")
    ro, runs, byo, vout, tot = out((B + 1) * 8, "run_offsets"), out(B * K * 8, "runs"), out((B * K + 1) * 8, "byte_offsets"), out(B * stride, "bytes_out"), out(32, "totals")
    ews = out(hra.extract_workspace_bytes(B), "workspace")
    cnt4 = _placed(alloc, torch.zeros(B, dtype=torch.int32, device=DEV), "span_counts").data_ptr()      # extract reads the counts: 4-byte aligned there
    sp_in = _placed(alloc, torch.zeros(B * K, dtype=torch.int64, device=DEV), "status_in").data_ptr()
    torch.cuda.synchronize()
    ctx, c, l, v, o, s, si = cfg._ctx, chars.data_ptr(), lens.data_ptr(), vals.data_ptr(), offs.data_ptr(), sel.data_ptr(), st_in.data_ptr()
    bounds = (C.c_uint32 * 2)(16, 64)

    def shifted(args):
        return lambda shift: tuple(x + shift[i] if i in shift else x for i, x in enumerate(args))
    total = 0
    total += _refusals("hrx_witness_batch_device_pitched", shifted((ctx, c, stride, l, B, M, rec, M, msk, M, st, None)), {1: 16, 3: 4, 6: 16, 8: 16, 10: 8}, alloc)
    for layout, src in ((1, c), (3, c)):
        total += _refusals("hrx_witness_batch_device_layout", shifted((ctx, layout, src, stride, l, B, M, rec, msk, st, None)), {2: 16, 4: 4, 7: 16, 8: 16, 9: 8}, alloc)
    for k in range(D):
        def planes_args(shift, k=k):
            arr = (C.c_void_p * D)(*[p + (shift.get("plane", 0) if j == k else 0) for j, p in enumerate(planes)])
            return (ctx, 1, c + shift.get(2, 0), stride, l + shift.get(4, 0), B, M, arr, D, msk + shift.get(9, 0), st + shift.get(10, 0), None)
        total += _refusals("hrx_witness_batch_device_planes", planes_args, {"plane": 16} if k else {2: 16, 4: 4, "plane": 16, 9: 16, 10: 8}, alloc)
    total += _refusals("hrx_match_batch_device", shifted((ctx, 0, c, stride, l, B, M, st, cnt, sp, K, None)), {2: 16, 4: 4, 7: 8, 8: 8, 9: 8}, alloc)
    total += _refusals("hrx_match_batch_device_ragged", shifted((ctx, v, o, B, M, st, cnt, sp, K, None)), {1: 16, 2: 8, 5: 8, 6: 8, 7: 8}, alloc)
    total += _refusals("hrx_match_selected_device", shifted((ctx, 0, c, stride, l, None, B, s, B, M, st, cnt, sp, K, None)), {2: 16, 4: 4, 7: 4, 10: 8, 11: 8, 12: 8}, alloc)
    total += _refusals("hrx_match_selected_device", shifted((ctx, hra.LAYOUT_INPUT_RAGGED, v, 0, None, o, B, s, B, M, st, cnt, sp, K, None)), {2: 16, 5: 8, 7: 4}, alloc)
    total += _refusals("hrx_ragged_to_position_major_device", shifted((ctx, v, o, B, stride, pm_out, lens_out, None)), {1: 16, 2: 8, 5: 16, 6: 4}, alloc)
    total += _refusals("hrx_gather_to_position_major_device", shifted((ctx, 0, c, stride, l, None, B, s, B, stride, pm_out, lens_out, None)), {2: 16, 4: 4, 7: 4, 10: 16, 11: 4}, alloc)
    total += _refusals("hrx_gather_to_position_major_device", shifted((ctx, hra.LAYOUT_INPUT_RAGGED, v, 0, None, o, B, s, B, stride, pm_out, lens_out, None)), {2: 16, 5: 8}, alloc)
    total += _refusals("hrx_chars_to_position_major_device", shifted((ctx, c, stride, B, pm_out, None)), {1: 16, 4: 16}, alloc)
    total += _refusals("hrx_route_device", shifted((ctx, si, 0, l, None, B, bounds, 2, order, bo, rws, hra.route_workspace_bytes(B), None)), {1: 8, 3: 4, 8: 4, 9: 8, 10: 8}, alloc)
    total += _refusals("hrx_route_device", shifted((ctx, si, 0, None, o, B, bounds, 2, order, bo, rws, hra.route_workspace_bytes(B), None)), {4: 8}, alloc)

    def extract_args(shift):
        eo = hra._ExtractOutC(ro + shift.get("ro", 0), runs + shift.get("runs", 0), byo + shift.get("bo", 0), vout, tot + shift.get("tot", 0), B * K, B * stride)
        return (ctx, hra.LAYOUT_INPUT_RAGGED, v, 0, o + shift.get(4, 0), B, si + shift.get(6, 0), cnt4 + shift.get(7, 0), sp_in + shift.get(8, 0), K, 0, C.byref(eo),
                ews + shift.get(12, 0), hra.extract_workspace_bytes(B), None)
    total += _refusals("hrx_extract_spans_device", extract_args, {4: 8, 6: 8, 7: 4, 8: 8, "ro": 8, "runs": 8, "bo": 8, "tot": 8, 12: 8}, alloc)
    assert total == 5 + 10 + 6 + 5 + 5 + 6 + 3 + 4 + 5 + 2 + 2 + 5 + 1 + 9
    alloc.check("the refusal matrix")
    # the witness entry names the rule that was broken (status 8-byte, lens 4-byte: not "16-byte aligned" for every output)
    for idx, word in ((10, "status 8-byte"), (3, "lens 4-byte"), (6, "records and masked must be 16-byte")):
        assert hra.lib.hrx_witness_batch_device_pitched(*shifted((ctx, c, stride, l, B, M, rec, M, msk, M, st, None))({idx: 2})) == hra.HRX_ERR_ARG
        assert word in hra.lib.hrx_last_error().decode(), hra.lib.hrx_last_error()
    # and the unshifted arguments are taken (the matrix is about the shift, nothing else)
    assert hra.lib.hrx_witness_batch_device_layout(ctx, 1, c, stride, l, B, M, rec, msk, st, None) == hra.HRX_OK
    torch.cuda.synchronize()
    assert not alloc.all_poison()


# =====================================================================================================================================================
# 2. stream order on a non-blocking side stream
# =====================================================================================================================================================
_RETURNS = []


def _side(cfg, alloc, delay):
    return cc.OnSideStream(torch, cfg, alloc, delay[0])


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_witness_rows_on_a_side_stream(hra, oracle, delay, row):
    """every row of the matrix and the forced chunked launch, one case each, every form of launch_every_form through the decoy protocol of
    caller_conditions.OnSideStream on a fresh non-blocking stream (buffers at minimum alignment, as in part 1)"""
    case = cc.stream_case(row)
    cfg = make_config(hra, row, case, 0)
    check_describe(row, cfg, case)
    want = expected(oracle, (row["id"], case.seed), case)
    tag = "%s seed %d (B=%d M=%d D=%d) on a side stream" % (row["id"], case.seed, case.B, case.M, case.D)
    alloc = cc.MinAlign(torch, DEV)
    side = _side(cfg, alloc, delay)
    s = torch.cuda.Stream(device=DEV)
    runs = launch_every_form(hra, row, case, side, want[0], want[3], tag, fr=bool(row.get("fr")) and case.D * case.B * case.M <= 1 << 18, alloc=alloc, stream=s)
    alloc.check(tag)
    assert side.calls >= len(runs) >= (1 if row["entry"] == "sm" else 2 if row.get("planes") is False else 3)
    _compare_runs(row, case, tag, want, runs)
    assert _flip_is_reported(row, case, want[3], want[1], want[2], runs[0])
    _RETURNS.extend(side.returns)


@pytest.mark.parametrize("name,flags", cc.MATCH_VARIANTS, ids=[v[0] for v in cc.MATCH_VARIANTS])
def test_match_ragged_and_selected_on_a_side_stream(oracle, delay, name, flags):
    case, want = _match_want(oracle, 2)
    cfg = _match_cfg(case, flags)
    _describe_match(cfg, case, name)
    sides = []

    def alloc_of():
        alloc = cc.MinAlign(torch, DEV)
        sides.append(_side(cfg, alloc, delay))
        return alloc

    class Cfg:          # each call through the protocol of the allocator made for it
        def __getattr__(self, attr):
            return getattr(sides[-1], attr)
    assert _every_match_form(Cfg(), case, want, alloc_of, stream=torch.cuda.Stream(device=DEV)) == 5
    assert sum(sd.calls for sd in sides) == 5
    for sd in sides:
        _RETURNS.extend(sd.returns)


def test_staging_route_and_extract_on_a_side_stream(delay):
    bt, cfg = _staging_batch(129)
    sides = []

    def alloc_of(poison=cc.POISON):
        alloc = cc.MinAlign(torch, DEV, poison)
        sides.append(_side(cfg, alloc, delay))
        return alloc

    class Cfg:
        def __getattr__(self, attr):
            return getattr(sides[-1], attr)
    assert _staging_calls(Cfg(), bt, alloc_of, stream=torch.cuda.Stream(device=DEV)) == 9
    assert sum(sd.calls for sd in sides) == 9
    for sd in sides:
        _RETURNS.extend(sd.returns)


def _handover(first, second, delay):
    """call 1 behind a delay on s1, then at once call 2 on s2, on the same context: when call 2 returns the event behind call 1 has completed (the host wait of
    include/hrx.h: "a launch on another stream first waits on the host for the stream that used the scratch last").  first(s) / second(s) prepare a call's buffers on
    its stream and return (go, read): go() is the library call alone, read() its result."""
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        go1, read1 = first(s1)
    with torch.cuda.stream(s2):
        go2, read2 = second(s2)
    torch.cuda.synchronize()          # (buffers made, inputs in place: from here on nothing but the delay, the two calls and the events)
    ev0, ev1 = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(s1):
        torch.cuda._sleep(delay[0])
        ev0.record(s1)
        go1()
        ev1.record(s1)
    open1 = not ev0.query()
    go2()
    waited = ev1.query()
    assert open1, "the delay had ended when call 1 returned: nothing to wait for"
    assert waited, "call 2 returned on another stream while call 1 of the same context was still using the scratch"
    s1.synchronize()
    s2.synchronize()
    return read1(), read2()


@pytest.mark.parametrize("row_id", cc.SCRATCH_ROWS)
def test_scratch_changes_streams_witness(hra, oracle, delay, row_id):
    """the chunked launch's scout / compose buffers, the multi-pass group buffers (merge and combine), the transpose buffers behind string-major outputs, the
    dynamic group counter: call 1 on one stream behind a delay, call 2 at once on another with the batch reversed and one string shorter"""
    row = cc.row_of(row_id)
    case = cc.stream_case(row)
    cfg = make_config(hra, row, case, 0)
    check_describe(row, cfg, case)
    o, orec, omsk, ost = expected(oracle, (row["id"], case.seed), case)
    sel2 = cc.handover_selection(case.B)
    d_chars, d_lens = torch.from_numpy(case.chars).to(DEV), torch.from_numpy(case.lens.astype(np.int32)).to(DEV)
    d_sel = torch.from_numpy(sel2).to(DEV)
    c2, l2 = d_chars.index_select(0, d_sel), d_lens.index_select(0, d_sel)
    form = "sm" if row["entry"] == "sm" else "pm-in"
    alloc = cc.MinAlign(torch, DEV)
    cc.launch_form(hra, torch, cfg, form, d_chars, d_lens, case.M, case.D, cc.MinAlign(torch, DEV))()      # eager: the scratch exists, at call 1's size
    got1, got2 = _handover(lambda s: cc.launch_form(hra, torch, cfg, form, d_chars, d_lens, case.M, case.D, alloc, s, defer=True),
                           lambda s: cc.launch_form(hra, torch, cfg, form, c2, l2, case.M, case.D, alloc, s, defer=True), delay)
    alloc.check(row_id + " handover")
    for tag, got, idx in (("call 1", got1, np.arange(case.B)), ("call 2", got2, sel2)):
        err = _compare(row, case, ost[idx], orec[idx], omsk[idx], *got)
        assert err is None, "%s %s: %s" % (row_id, tag, err)


def test_scratch_changes_streams_match_via_rows(oracle, delay):
    """via-rows match: the witness rows go into context scratch"""
    case, want = _match_want(oracle, 2)
    cfg = _match_cfg(case, 1 << 32)
    assert cfg.describe_match(case.B).startswith("via rows")
    K, B = cc.MATCH_SPANS, case.B
    sel2 = cc.handover_selection(B)
    d_chars, d_lens = torch.from_numpy(case.chars).to(DEV), torch.from_numpy(case.lens.astype(np.int32)).to(DEV)
    d_sel = torch.from_numpy(sel2).to(DEV)
    c2, l2 = d_chars.index_select(0, d_sel), d_lens.index_select(0, d_sel)
    cfg.match_batch(d_chars, d_lens, max_spans=K)
    alloc = cc.MinAlign(torch, DEV)

    def call(c, l):
        def go(s):
            n = l.numel()
            out = (alloc(n * 8, torch.int64, "status")[0], alloc(n * 4, torch.int32, "counts")[0], alloc(n * K * 8, torch.int64, "spans")[0].view(n, K))
            pc, pl = _placed(alloc, c, "chars"), _placed(alloc, l, "lens")
            return (lambda: cfg.match_batch(pc, pl, max_spans=K, out=out, stream=s)), (lambda: tuple(t.cpu().numpy().view(dt) for t, dt in zip(out, (np.uint64, np.uint32, np.uint64))))
        return go
    got1, got2 = _handover(call(d_chars, d_lens), call(c2, l2), delay)
    alloc.check("via-rows handover")
    ost, (ecnt, eruns) = want
    check_match(got1, want, K)
    check_match(got2, (ost[sel2], ([ecnt[b] for b in sel2], [eruns[b] for b in sel2])), K)


# =====================================================================================================================================================
# 3. one long-lived context, changing batch sizes
# =====================================================================================================================================================
def _forms(row):
    if row["entry"] == "sm":
        return ["sm", "sm-pitched"]
    return ["pm", "pm-in"] + ([] if row.get("planes") is False else ["planes", "planes-in"])


@pytest.mark.parametrize("row_id", cc.SEQUENCE_ROWS)
def test_one_context_over_changing_batch_sizes(hra, oracle, row_id):
    """B = 129, 1, 65, 320 (beyond reserve()'s 1.25 x headroom: the scratch regrows), 64, 129 again and 0 on ONE context and one side stream, the output forms the
    row admits in turn, nothing synchronized between the calls; every call's rows compared after the one synchronize at the end"""
    row = cc.row_of(row_id)
    case = cc.sequence_case(row)
    o, orec, omsk, ost = expected(oracle, ("sequence", row_id), case)
    sizes = cc.sequence_sizes(row, case)
    assert case.B >= max(sizes)
    cfg = make_config(hra, row, case, 0)
    if max(sizes) == case.B:
        check_describe(row, cfg, case)
    sels = [cc.selection(case, ost, omsk, k, n) for k, n in enumerate(sizes)]
    forms = _forms(row)
    s = torch.cuda.Stream(device=DEV)
    alloc = cc.MinAlign(torch, DEV)
    d_chars, d_lens = torch.from_numpy(case.chars).to(DEV), torch.from_numpy(case.lens.astype(np.int32)).to(DEV)
    d_sels = [torch.from_numpy(x).to(DEV) for x in sels]
    torch.cuda.synchronize()
    readers = []
    with torch.cuda.stream(s):
        for k, d_sel in enumerate(d_sels):
            readers.append(cc.launch_form(hra, torch, cfg, forms[k % len(forms)], d_chars.index_select(0, d_sel), d_lens.index_select(0, d_sel), case.M, case.D, alloc, s))
    s.synchronize()
    alloc.check(row_id + " sequence")
    live = False
    for k, (read, idx) in enumerate(zip(readers, sels)):
        got = read()
        assert got[0].shape == (len(idx),)
        if len(idx) == 0:          # B == 0: HRX_OK (the call returned), nothing to write, and the guards of its empty buffers are intact
            continue
        err = _compare(row, case, ost[idx], orec[idx], omsk[idx], *got)
        assert err is None, "%s call %d (B=%d, %s): %s" % (row_id, k, len(idx), forms[k % len(forms)], err)
        if not live and len(idx) > 1:
            live = _flip_is_reported(row, case, ost[idx], orec[idx], omsk[idx], (None,) + got)
    assert live


# =====================================================================================================================================================
def test_the_delay_and_the_host_return_times(delay):
    """the figures the side-stream tests rest on, printed (pytest -s): the delay by the device's events, and how long the warm calls and the calls behind the
    delay took to return to the host"""
    cycles, ms = delay
    t0 = time.perf_counter()
    torch.cuda.synchronize()
    print("\ndelay: torch.cuda._sleep(%d) = %.3f ms by events" % (cycles, ms))
    if _RETURNS:
        warm = np.array([w for _, w, _ in _RETURNS]) * 1e6
        side = np.array([x for _, _, x in _RETURNS]) * 1e6
        print("host return time of %d calls: warm (default stream) median %.1f us, max %.1f us; behind the delay median %.1f us, max %.1f us" % (
            len(_RETURNS), float(np.median(warm)), float(warm.max()), float(np.median(side)), float(side.max())))
        assert float(side.max()) * 1e-3 < ms, "a call took longer to return than the delay lasts"
    assert time.perf_counter() - t0 < 5
