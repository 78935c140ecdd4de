"""EXTRACT on the host (include/hrx.h: hrx_extract_spans_host behind extract_batch_host / extract_batch_host_ragged / extract_strings, host-only contexts):
the list column of revealed bytes against an expectation that never touches the code under test — the oracle's masked rows, run-length encoded by
rle_masked, the bytes sliced out of the test's own copy of the input, concatenated and summed in numpy.  Everything bit for bit."""
import functools
import os
import subprocess

import numpy as np
import pytest

import carry_defs as cd
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import OracleDefs, ROOT, load_oracle, reference_cases
from test_match_cpu import CFG_A, _cfg, _defs, rle_masked

POISON64, POISON8 = np.uint64(0x5A5A5A5A5A5A5A5A), np.uint8(0x5A)
GUARD = 16          # poisoned words / bytes behind every cap


def lever_cfg(case, device=hra.HRX_DEVICE_NONE):
    defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
    return hra.RegexVerifyConfig.configure(case.M, defs, device=device)


class Batch:
    """a batch with the oracle's answer: chars, lens, M, the oracle's status and rle_masked's (counts, runs); make_cfg(device) -> its config"""

    def __init__(self, name, chars, lens, M, ost, ecnt, eruns, make_cfg):
        self.name, self.chars, self.lens, self.M, self.ost, self.ecnt, self.eruns, self.make_cfg = name, chars, lens, M, ost, ecnt, eruns, make_cfg

    def prefix(self, B):
        return Batch(self.name, self.chars[:B], self.lens[:B], self.M, self.ost[:B], self.ecnt[:B], self.eruns[:B], self.make_cfg)


def _lever(name, min_batch=0, **kw):
    case = cd.scenario_batch(cap=4, min_batch=min_batch, **kw)
    o = OracleDefs(load_oracle(), [(a, subs) for a, subs, _ in case.defs_t])
    _, omsk, ost = o.witness_batch(case.chars, case.lens, case.M, threads=16)
    ecnt, eruns = rle_masked(omsk, case.lens, ost)
    return Batch(name, case.chars, case.lens, case.M, ost, ecnt, eruns, functools.partial(lever_cfg, case))


@functools.lru_cache(maxsize=None)
def batch(name):
    """computed once per session and never changed"""
    if name == "lever256":
        return _lever(name, M=256)
    if name == "lever256_second":
        return _lever(name, M=256, D=2, second=True)
    if name == "lever1001":
        return _lever(name, M=1001, D=3)
    if name == "lever_border":                  # tiles itself past 70001 strings: crosses a position-major block
        return _lever(name, M=256, D=2, second=True, min_batch=70001)
    if name.startswith("stress"):               # stress256: reveal_stress(2000, 256, seed=9); stress64_N: N strings of 64 rows
        M, B = (256, 2000) if name == "stress256" else (64, int(name.split("_")[1]))
        chars, lens = synth.reveal_stress(B, M, seed=9)
        _, omsk, ost = OracleDefs.from_files(load_oracle(), CFG_A).witness_batch(chars, lens, M, threads=16)
        ecnt, eruns = rle_masked(omsk, lens, ost)
        return Batch(name, chars, lens, M, ost, ecnt, eruns, lambda device=hra.HRX_DEVICE_NONE: _cfg(CFG_A, M, device=device))
    raise KeyError(name)


BATCHES = ["lever256", "lever256_second", "lever1001", "stress256"]


def expect(bt, max_spans, require_accept=0):
    """(run_offsets, runs, byte_offsets, values, totals) as include/hrx.h EXTRACT defines them, from the oracle's runs and the test's own bytes"""
    B = len(bt.lens)
    run_offsets = np.zeros(B + 1, np.uint64)
    words, lengths, parts, trunc = [], [], [], 0
    for b in range(B):
        s = int(bt.ost[b])
        if (s & 0xff) == 0 and ((s >> 8) & require_accept) == require_accept:
            trunc += bt.ecnt[b] > max_spans
            for sid, start, ln in bt.eruns[b][:max_spans]:
                words.append(start | ln << 28 | sid << 56)
                lengths.append(ln)
                parts.append(bt.chars[b, start:start + ln])
        run_offsets[b + 1] = len(words)
    byte_offsets = np.concatenate((np.zeros(1, np.uint64), np.cumsum(np.array(lengths, np.uint64), dtype=np.uint64)))
    values = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return run_offsets, np.array(words, np.uint64), byte_offsets, values, np.array([len(words), len(values), trunc, 0], np.uint64)


def check_full(ex, want):
    """an Extracted of numpy arrays whose caps sufficed == the expectation"""
    ro, runs, bo, vals, tot = want
    R, nb = len(runs), len(vals)
    assert np.array_equal(ex.totals, tot), (ex.totals, tot)
    assert np.array_equal(ex.run_offsets, ro)
    assert np.array_equal(ex.runs[:R], runs) and np.array_equal(ex.byte_offsets[:R + 1], bo) and np.array_equal(ex.values[:nb], vals)


def stored_prefix(want, runs_cap, values_cap):
    """J of the capacity rule: run j is stored iff j < runs_cap and byte_offsets[j + 1] <= values_cap"""
    _, runs, bo, _, _ = want
    J = 0
    while J < min(len(runs), runs_cap) and int(bo[J + 1]) <= values_cap:
        J += 1
    return J


def check_capped(got, want, runs_cap, values_cap):
    """got = (run_offsets, runs, byte_offsets, values, totals) with GUARD poisoned elements behind runs_cap / runs_cap + 1 / values_cap and poison written
    everywhere before the call: totals and run_offsets complete, the stored prefix [0, J) exact, nothing else touched"""
    ro, runs, bo, vals, tot = got
    wro, wruns, wbo, wvals, wtot = want
    J = stored_prefix(want, runs_cap, values_cap)
    assert np.array_equal(tot, wtot) and np.array_equal(ro, wro)
    assert np.array_equal(runs[:J], wruns[:J]) and np.array_equal(bo[:J + 1], wbo[:J + 1])
    nb = int(wbo[J])
    assert np.array_equal(vals[:nb], wvals[:nb])
    assert (runs[J:] == POISON64).all() and (bo[J + 1:] == POISON64).all() and (vals[nb:] == POISON8).all()
    assert len(runs) == runs_cap + GUARD and len(bo) == runs_cap + 1 + GUARD and len(vals) == values_cap + GUARD
    return J


def poisoned_out(B, runs_cap, values_cap):
    """-> (the five arrays as the call takes them, the five with their guards)"""
    full = (np.full(B + 1 + GUARD, POISON64), np.full(runs_cap + GUARD, POISON64), np.full(runs_cap + 1 + GUARD, POISON64),
            np.full(values_cap + GUARD, POISON8), np.full(4 + GUARD, POISON64))
    return (full[0][:B + 1], full[1][:runs_cap], full[2][:runs_cap + 1], full[3][:values_cap], full[4][:4]), full


def column(chars, lens, lead=0):
    """the strings chars[b, :lens[b]] back to back after `lead` bytes, 16-byte padded, filled with 0xAA elsewhere (tests/test_ragged_gpu.py _column)"""
    L = np.minimum(lens.astype(np.int64), chars.shape[1])
    offsets = np.zeros(len(L) + 1, np.int64)
    np.cumsum(L, out=offsets[1:])
    offsets += lead
    values = np.full(-(-int(offsets[-1]) // 16) * 16 + 16, 0xAA, np.uint8)
    values[lead:int(offsets[-1])] = chars[np.arange(chars.shape[1])[None, :] < L[:, None]]
    return values, offsets.astype(np.uint64)


def short_caps(want):
    """(runs_cap, values_cap) pairs: exact, one below need on either side, interior values, a values_cap inside a run, nothing"""
    _, runs, bo, _, _ = want
    R, nb = len(runs), int(bo[-1])
    mid = R // 2
    inside = next(int(bo[j]) + 1 for j in range(mid + 1, R) if int(bo[j + 1]) - int(bo[j]) >= 2)        # one byte into a run of two bytes or more
    return [(R, nb), (R - 1, nb), (R, nb - 1), (mid, nb), (R, int(bo[mid])), (R, inside), (3, 5), (0, nb), (R, 0), (0, 0)]


@pytest.mark.parametrize("max_spans", [1, 4, 16])
@pytest.mark.parametrize("name", BATCHES)
def test_parity_with_the_oracle(name, max_spans):
    bt = batch(name)
    cfg = bt.make_cfg()
    want = expect(bt, max_spans)
    ex = cfg.extract_batch_host(bt.chars, bt.lens, max_spans=max_spans)
    check_full(ex, want)
    assert int(ex.totals[2]) == sum(1 for b in range(len(bt.lens)) if not int(bt.ost[b]) & 0xff and bt.ecnt[b] > max_spans)
    assert hra.extracted_lists(ex) == hra.revealed_substrings(bt.chars, bt.lens, ex.status, ex.counts, cfg.match_batch_host(bt.chars, bt.lens, max_spans=max_spans)[2])
    values, offsets = column(bt.chars, bt.lens, lead=3)
    exr = cfg.extract_batch_host_ragged(values, offsets, max_spans=max_spans)
    keep = bt.lens <= bt.M                               # (a string longer than M has status 3 either way)
    assert np.array_equal(exr.status[keep], bt.ost[keep])
    check_full(exr, want)
    assert hra.extracted_lists(exr) == hra.extracted_lists(ex)


def test_the_batches_hold_the_cases_they_are_chosen_for():
    """what the oracle says about the batches (nothing of the code under test): bad statuses, strings over a cap of 4, long runs, every accept mask"""
    facts = {}
    for name in BATCHES:
        bt = batch(name)
        code = bt.ost & np.uint64(0xff)
        facts[name] = (len(bt.lens), int((code != 0).sum()), sum(c > 4 for c in bt.ecnt), max(c for c in bt.ecnt), max(r[2] for rs in bt.eruns for r in rs))
    assert facts["lever256"] == (193, 2, 1, 9, 249)
    assert facts["lever256_second"][:3] == (212, 4, 2)
    assert facts["lever1001"][0] == 240 and facts["lever1001"][3] == 29 and facts["lever1001"][4] == 994
    st = batch("stress256")
    assert facts["stress256"][2] == 3 and int(expect(st, 1 << 16)[4][1]) == 71573
    assert set(((st.ost[(st.ost & np.uint64(0xff)) == 0] >> np.uint64(8)) & np.uint64(3)).tolist()) == {0, 1, 2, 3}


CASES = [c for c in reference_cases() if c["masked_outputs_asserted"]]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_expected_substrs(case):
    """lib.rs:1046-1058: extract_strings gives the reference's own expected_substrs, ids 1, 2, ... in list order"""
    cfg = _cfg(case["defs"], case["max_chars_size"])
    ex = cfg.extract_strings([case["input"].encode("latin-1")])
    assert hra.extracted_lists(ex)[0] == [(k + 1, start, text.encode("latin-1")) for k, (start, text) in enumerate(case["expected_substrs"])]


@pytest.mark.parametrize("mask", [1, 2, 3])
def test_require_accept(mask):
    bt = batch("stress256")
    cfg = bt.make_cfg()
    want = expect(bt, 16, require_accept=mask)
    ex = cfg.extract_batch_host(bt.chars, bt.lens, max_spans=16, require_accept=mask)
    check_full(ex, want)
    k = np.diff(ex.run_offsets.astype(np.int64))
    covers = ((bt.ost & np.uint64(0xff)) == 0) & (((bt.ost >> np.uint64(8)) & np.uint64(mask)) == np.uint64(mask))
    assert not k[~covers].any() and (k[covers] == np.minimum(np.array(bt.ecnt), 16)[covers]).all()
    assert 0 < int(covers.sum()) < len(covers) and int(want[4][0]) < int(expect(bt, 16)[4][0])
    assert hra.extracted_column(ex, 1)[1][-1] + hra.extracted_column(ex, 2)[1][-1] == int(want[4][1])


@pytest.mark.parametrize("ragged", [False, True], ids=["padded", "ragged"])
def test_short_caps(ragged):
    bt = batch("stress256")
    cfg = bt.make_cfg()
    want = expect(bt, 4)
    values, offsets = column(bt.chars, bt.lens, lead=5)
    B = len(bt.lens)
    seen = set()
    for runs_cap, values_cap in short_caps(want):
        out, full = poisoned_out(B, runs_cap, values_cap)
        if ragged:
            cfg.extract_batch_host_ragged(values, offsets, max_spans=4, out=out)
        else:
            cfg.extract_batch_host(bt.chars, bt.lens, max_spans=4, out=out)
        seen.add(check_capped((full[0][:B + 1], full[1], full[2], full[3], full[4][:4]), want, runs_cap, values_cap))
        assert (full[0][B + 1:] == POISON64).all() and (full[4][4:] == POISON64).all()
    assert len(seen) >= 5 and 0 in seen and len(want[1]) in seen              # several different prefixes, none and all among them
    # the caller reads totals and comes back with exact caps: everything
    ex = cfg.extract_batch_host(bt.chars, bt.lens, max_spans=4, caps=(int(want[4][0]), int(want[4][1])))
    check_full(ex, want)
    assert len(ex.runs) == int(want[4][0]) and len(ex.values) == int(want[4][1])


def _word(start, length, sid=1):
    return start | length << 28 | sid << 56


def test_clipping_of_hand_made_span_words():
    """span words are caller memory: a run that leaves its slot / its ragged string is clipped to it, decreasing offsets contribute nothing"""
    stride = 32
    chars = np.arange(3 * stride, dtype=np.uint8).reshape(3, stride)
    status = np.array([1 << 8, 1 << 8, 1 << 8], np.uint64)
    counts = np.array([2, 1, 1], np.uint32)
    spans = np.array([[_word(4, 3), _word(30, 9, 2)], [_word(40, 5), 0], [_word(0, (1 << 28) - 1), 0]], np.uint64)
    ex = hra.extract_spans_host(chars, status, counts, spans)
    assert ex.totals.tolist() == [4, 3 + 2 + 0 + 32, 0, 0] and ex.run_offsets.tolist() == [0, 2, 3, 4]
    assert ex.byte_offsets[:5].tolist() == [0, 3, 5, 5, 37]                    # 9 rows from row 30 of a 32-byte slot: 2; a run that starts past the slot: 0
    assert np.array_equal(ex.runs[:4], spans[[0, 0, 1, 2], [0, 1, 0, 0]])      # the words as given
    assert bytes(ex.values[:37]) == bytes(chars[0, 4:7]) + bytes(chars[0, 30:32]) + bytes(chars[2])
    # ragged: string 0 = 10 bytes, string 1 has decreasing offsets, string 2 = 6 bytes
    values = np.arange(64, dtype=np.uint8)
    offsets = np.array([3, 13, 9, 15], np.uint64)
    spans = np.array([[_word(8, 5), _word(2, 2, 3)], [_word(0, 4), 0], [_word(5, 100), 0]], np.uint64)
    ex = hra.extract_spans_host(values, status, counts, spans, offsets=offsets)
    assert ex.totals.tolist() == [3, 2 + 2 + 1, 0, 0] and ex.run_offsets.tolist() == [0, 2, 2, 3]
    assert ex.byte_offsets[:4].tolist() == [0, 2, 4, 5]
    assert bytes(ex.values[:5]) == bytes(values[11:13]) + bytes(values[5:7]) + bytes(values[14:15])
    assert hra.extracted_lists(ex) == [[(1, 8, bytes(values[11:13])), (3, 2, bytes(values[5:7]))], [], [(1, 5, bytes(values[14:15]))]]


def test_argument_errors():
    bt = batch("stress256").prefix(8)
    cfg = bt.make_cfg()
    st, cnt, sp = cfg.match_batch_host(bt.chars, bt.lens, max_spans=4)

    def code(fn):
        with pytest.raises(hra.HrxError) as e:
            fn()
        return e.value.code

    assert code(lambda: hra.extract_spans_host(bt.chars, st, cnt, sp[:, :0])) == hra.HRX_ERR_ARG                      # max_spans = 0
    buf = np.zeros(4 * 8 + 8, np.uint8)
    odd = buf[4:4 + 32].view(np.uint64)                                                                              # 4 mod 8
    good = lambda: [np.zeros(9, np.uint64), np.zeros(32, np.uint64), np.zeros(33, np.uint64), np.zeros(bt.chars.size, np.uint8), np.zeros(4, np.uint64)]
    o = good()
    o[4] = odd
    assert code(lambda: hra.extract_spans_host(bt.chars, st, cnt, sp, out=o)) == hra.HRX_ERR_ARG                      # misaligned totals
    import ctypes as C
    out = hra._ExtractOutC(0, 0, 0, 0, 0, 0, 0)
    args = (hra.LAYOUT_STRING_MAJOR, bt.chars.ctypes.data, bt.chars.shape[1], None, 8, st.ctypes.data, cnt.ctypes.data, sp.ctypes.data, 4, 0)
    assert hra.lib.hrx_extract_spans_host(*args, C.byref(out), 1) == hra.HRX_ERR_ARG                                   # NULL outputs
    assert hra.lib.hrx_extract_spans_host(*args, None, 1) == hra.HRX_ERR_ARG
    assert hra.lib.hrx_extract_spans_host(hra.LAYOUT_INPUT_POSITION_MAJOR, *args[1:], C.byref(out), 1) == hra.HRX_ERR_ARG   # the host form: no position-major input
    o = good()
    ok = hra._ExtractOutC(*[a.ctypes.data for a in o], 32, bt.chars.size)
    ws = np.zeros(hra.extract_workspace_bytes(8) // 8, np.uint64)
    dev_args = (cfg._ctx,) + args
    assert hra.lib.hrx_extract_spans_device(*dev_args, C.byref(ok), ws.ctypes.data, ws.nbytes - 8, None) == hra.HRX_ERR_ARG    # workspace too small
    assert hra.lib.hrx_extract_spans_device(*dev_args, C.byref(ok), ws.ctypes.data, ws.nbytes, None) == hra.HRX_ERR_HIP        # a host-only context
    assert hra.lib.hrx_extract_spans_device(None, *args, C.byref(ok), ws.ctypes.data, ws.nbytes, None) == hra.HRX_ERR_ARG
    assert hra.extract_workspace_bytes(0) >= 32 and hra.extract_workspace_bytes(1 << 20) < (1 << 20)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_extract_host.cpp: csrc/hrx_extract.hpp + csrc/hrx_extract_host.cpp compiled into a program of their own with the address and
    undefined-behaviour sanitizers: short caps with exactly sized heap arrays (a byte too far is an error there), clipped runs, decreasing offsets, threads"""
    exe = str(tmp_path / "hrx_test_extract_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_extract_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "extract host: ok" in out.stdout, out.stdout + out.stderr
