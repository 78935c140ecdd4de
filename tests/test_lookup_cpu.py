"""LOOKUP COUNTS on the host (include/hrx.h hrx_lookup_counts_host on host-only contexts; csrc/hrx_lookup.hpp): the counts against tests/lookup_ref.py — table rows
and cells from the oracle, tuples as src/lib.rs writes them, a dict lookup — on rows produced by witness_batch_host in every host row form; the sums a prover
relies on; duplicate endpoint rows; tampered rows against the verdict of hrx_verify_rows_host; the contract; permuted_lookup_columns; and the rule as a program
of its own under the sanitizers.  No device."""
import os
import subprocess

import numpy as np
import pytest

import halo2_regex_amd as hra
from halo2_regex_amd import synth
from lookup_ref import LookupRef
from oracle_lib import OracleDefs, ROOT
from test_match_cpu import CFG_1, CFG_A, CFG_3, CFG_23, CFG_H4, _cfg

CFG_123 = CFG_A + CFG_3
LOOKUP_BITS = hra.VERIFY_TRANSITION | hra.VERIFY_START_LOOKUP | hra.VERIFY_END_LOOKUP
SETS = {"regex1": CFG_1, "regex12": CFG_A, "regex123": CFG_123, "headers4": CFG_H4}
TEXT = b"email was meant for @yajk. Also for swq.\r\nfrom:alice<a@b.com>\r\nto:bob<b@c.com>\r\nsubject:Send 1 ETH to z@y.com\r\n"


def small_batch(M):
    """strings of n = 0, 1, M - 1, M characters (each twice: a piece of TEXT from its start, and one from the e-mail literal on), and ragged noise with plants"""
    chars, lens = synth.ragged(8, M, seed=M)
    ns = sorted({0, min(1, M), M - 1, M})
    B = 2 * len(ns) + len(lens)
    out = np.zeros((B, max(16, (M + 15) // 16 * 16)), np.uint8)
    ln = np.zeros(B, np.uint32)
    for k, n in enumerate(ns):
        for j, text in enumerate((TEXT, TEXT[20:])):
            out[2 * k + j, :n] = np.frombuffer((text * (n // len(text) + 1))[:n], np.uint8)
            ln[2 * k + j] = n
    out[2 * len(ns):, :chars.shape[1]] = chars[:, :out.shape[1]]
    ln[2 * len(ns):] = np.minimum(lens, M)
    return out, ln


def to_position_major(rec, M, D):
    B = rec.shape[0]
    assert B <= hra.PM_BLOCK
    q4 = (M + 3) // 4
    r4 = np.zeros((B, q4 * 4, D), np.uint32)
    r4[:, :M] = rec
    return np.ascontiguousarray(r4.reshape(B, q4, 4, D).transpose(1, 3, 0, 2)).reshape(-1)


def check_against_ref(cfg, ref, chars, lens, rec, st, counts, misses, sample=None):
    M, lay = cfg.max_chars_size, cfg.lookup_layout()
    assert lay == ref.layout() and counts.shape[1] == ref.words() == cfg.lookup_words() and ref.words() % 4 == 0
    for b in (range(len(lens)) if sample is None else sample):
        n = int(lens[b])
        run, miss = ref.count_records(chars[b], n, M, rec[b])
        assert np.array_equal(counts[b], run), "string %d (n = %d)" % (b, n)
        assert int(misses[b]) == miss.sum()
        for d in range(cfg.num_defs):
            assert counts[b][lay[d]["trans"]].sum() + miss[d, 0] == M - (n == M)
            assert counts[b][lay[d]["start"]].sum() + miss[d, 1] == M
            assert counts[b][lay[d]["end"]].sum() + miss[d, 2] == M - (n == M)
        if int(st[b]) & 0xff == 0:          # clean rows: the oracle's own cells give the same run and nothing is missed
            run2, miss2 = ref.count_string(bytes(chars[b, :n]), M)
            assert np.array_equal(run2, run) and not miss2.any() and int(misses[b]) == 0
            for d in range(cfg.num_defs):
                assert counts[b][lay[d]["start"]].sum() == M


@pytest.mark.parametrize("M", [1, 3, 4, 5, 19, 64])
@pytest.mark.parametrize("name", list(SETS))
def test_host_twin_against_the_reference_in_every_row_form(oracle, name, M):
    cfg = _cfg(SETS[name], M)
    ref = LookupRef(OracleDefs.from_files(oracle, SETS[name]))
    chars, lens = small_batch(M)
    B, D = len(lens), cfg.num_defs
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    assert (st & np.uint64(0xff) == 0).sum() >= 2
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    check_against_ref(cfg, ref, chars, lens, rec, st, counts, misses)
    # a pitched view, the position-major image, position-major input: the same words
    rp = np.full((B, M + 40, D), 0xffffffff, np.uint32)
    rp[:, :M] = rec
    c2, m2 = cfg.lookup_counts_host(chars, lens, rp[:, :M])
    assert np.array_equal(c2, counts) and np.array_equal(m2, misses)
    rec_pm = to_position_major(rec, M, D)
    c3, m3 = cfg.lookup_counts_host(chars, lens, rec_pm, layout=hra.LAYOUT_POSITION_MAJOR)
    assert np.array_equal(c3, counts) and np.array_equal(m3, misses)
    c4, m4 = cfg.lookup_counts_host(hra.chars_to_position_major(chars), lens, rec_pm, layout=hra.LAYOUT_POSITION_MAJOR | hra.LAYOUT_INPUT_POSITION_MAJOR,
                                    chars_pm_stride=chars.shape[1])
    assert np.array_equal(c4, counts) and np.array_equal(m4, misses)


def test_duplicate_endpoint_rows_the_lowest_takes_the_count(oracle):
    """a start_states list that names state 0 twice: two endpoint rows (1, 0, dummy); the lower one is counted, the other stays 0"""
    allstr = "0\n2\n2\n0 1 97\n1 1 98\n1 2 97\n2 2 97\n"
    sub = "4\n0\n7\n0 0\n1\n0 1\n1 1\n"
    cfg = hra.RegexVerifyConfig.configure(8, [hra.RegexDefs(hra.AllstrRegexDef(allstr), [hra.SubstrRegexDef(sub)])], device=hra.HRX_DEVICE_NONE)
    ep = [tuple(int(v) for v in r) for r in cfg.load()[0][1]]
    assert ep == [(0, 3, 3), (1, 0, 3), (1, 0, 3), (1, 3, 1)]
    chars = np.zeros((1, 16), np.uint8)
    chars[0, :4] = np.frombuffer(b"abba", np.uint8)
    lens = np.array([4], np.uint32)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    assert int(st[0]) & 0xff == 0 and int(rec[0, 0, 0]) >> 24 & 1 == 1
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    lay = cfg.lookup_layout()[0]
    assert counts[0][lay["start"]].tolist() == [7, 1, 0, 0] and misses[0] == 0
    ref = LookupRef(OracleDefs(oracle, [(allstr.encode(), [sub.encode()])]))
    check_against_ref(cfg, ref, chars, lens, rec, st, counts, misses)


def tampered(rec, n, M):
    """(name, rows) per mutation of one string's records (M, D): states, ids, flags, values outside every table"""
    def mut(fn):
        r = rec.copy()
        fn(r)
        return r
    u = np.uint32
    def state(r): r[10, 0] = (r[10, 0] & u(0xffff0000)) | u(3)
    def sid(r): r[3, 0] |= u(1 << 16)
    def start(r): r[22, 0] |= u(1 << 24)
    def end_ok(r): r[21, 0] |= u(1 << 25)
    def end_bad(r): r[20, 0] |= u(1 << 25)
    def drop_start(r): r[21, 0] &= ~u(1 << 24)
    def pad_state(r): r[100, 0] = 0
    def pad_flag(r): r[M - 1, 1] |= u(3 << 24)
    def big_state(r): r[5, 1] |= u(0xffff)
    def big_state_pad(r): r[n + 3, 0] |= u(0xffff)
    def big_sid(r): r[7, 0] |= u(0xff << 16) | u(1 << 24)
    def big_flags(r): r[9, 1] |= u(0xfc << 24)
    def all_ones(r): r[30, :] = u(0xffffffff)
    return [(f.__name__, mut(f)) for f in (state, sid, start, end_ok, end_bad, drop_start, pad_state, pad_flag, big_state, big_state_pad, big_sid, big_flags, all_ones)]


def test_tampered_rows_miss_exactly_where_verify_reports_a_lookup(oracle):
    M = 128
    s = b"email was meant for @yajk. Also for swq."
    n = len(s)
    cfg = _cfg(CFG_A, M)
    ref = LookupRef(OracleDefs.from_files(oracle, CFG_A))
    base = np.zeros((1, 48), np.uint8)
    base[0, :n] = np.frombuffer(s, np.uint8)
    rec0, msk0, st0 = cfg.witness_batch_host(base, np.array([n], np.uint32))
    cases = [("clean", rec0[0])] + tampered(rec0[0], n, M)
    B = len(cases)
    chars, lens = np.repeat(base, B, 0), np.full(B, n, np.uint32)
    rec = np.stack([r for _, r in cases])
    msk = np.repeat(msk0, B, 0)
    verdict = cfg.verify_rows_host(chars, lens, rec, msk)
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    seen = 0
    for b, (name, _) in enumerate(cases):
        assert (misses[b] != 0) == (int(verdict[b]) & LOOKUP_BITS != 0), (name, hra.explain_verdict(verdict[b]), int(misses[b]))
        run, miss = ref.count_records(chars[b], n, M, rec[b])
        assert np.array_equal(counts[b], run) and int(misses[b]) == miss.sum(), name
        for k, bit in enumerate((hra.VERIFY_TRANSITION, hra.VERIFY_START_LOOKUP, hra.VERIFY_END_LOOKUP)):
            assert (miss[:, k].sum() != 0) == (int(verdict[b]) & bit != 0), (name, k)
        seen |= int(verdict[b]) & LOOKUP_BITS
    # a valid end flag, a dropped start flag (its tuple becomes the dummy row), whatever sits in a disabled row's state, flag bits above the two, and the
    # two flags on a padding row (their tuples are the dummy row's) are in the tables; the rest is not
    assert seen == LOOKUP_BITS and {name for (name, _), m in zip(cases, misses) if m} == {"state", "sid", "start", "end_bad", "big_state", "big_sid", "all_ones"}


def test_contract_of_the_host_form(oracle):
    M, B = 64, 40
    cfg = _cfg(CFG_A, M)
    chars, lens = synth.ragged(B, M, seed=1)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    W = cfg.lookup_words()
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    assert counts.shape == (B, W) and W == hra.lib.hrx_lookup_words_per_string(cfg._defs.h)
    lay = cfg.lookup_layout()
    used = sum(l["end"].stop - l["trans"].start for l in lay)
    assert lay[0]["trans"].start == 0 and lay[1]["trans"].start == lay[0]["end"].stop and used <= W < used + 4 and not counts[:, used:].any()
    for d, (tr, ep) in enumerate(cfg.load()):
        assert lay[d]["trans"].stop - lay[d]["trans"].start == len(tr) and lay[d]["start"].stop - lay[d]["start"].start == len(ep) == lay[d]["end"].stop - lay[d]["end"].start
    # n > M: every bin 0, misses all ones; the others unchanged
    long_lens = lens.copy()
    long_lens[3] = M + 1
    c2, m2 = cfg.lookup_counts_host(chars, long_lens, rec)
    assert not c2[3].any() and m2[3] == 0xffffffff and np.array_equal(np.delete(c2, 3, 0), np.delete(counts, 3, 0)) and np.array_equal(np.delete(m2, 3), np.delete(misses, 3))
    # the window: between poisoned guards, the strings' own words; misses may be NULL
    G = 1024
    for b_begin, b_count in ((0, B), (5, 9), (B - 1, 1), (7, 0)):
        raw = np.full(G + b_count * W + G, 0x5A5A5A5A, np.uint32)
        rawm = np.full(G + b_count + G, 0x5A5A5A5A, np.uint32)
        out, mo = raw[G:G + b_count * W].reshape(b_count, W), rawm[G:G + b_count]
        if b_count:
            cfg.lookup_counts_host(chars, lens, rec, b_begin=b_begin, b_count=b_count, out=out, misses=mo)
        else:
            assert hra.lib.hrx_lookup_counts_host(cfg._ctx, 0, chars.ctypes.data, chars.shape[1], lens.ctypes.data, rec.ctypes.data, 0, B, M, b_begin, 0, None, None) == hra.HRX_OK
        assert np.array_equal(out, counts[b_begin:b_begin + b_count]) and np.array_equal(mo, misses[b_begin:b_begin + b_count])
        assert (raw[:G] == 0x5A5A5A5A).all() and (raw[G + b_count * W:] == 0x5A5A5A5A).all() and (rawm[:G] == 0x5A5A5A5A).all() and (rawm[G + b_count:] == 0x5A5A5A5A).all()
    out = np.full((B, W), 0x5A5A5A5A, np.uint32)
    args = (chars.ctypes.data, chars.shape[1], lens.ctypes.data, rec.ctypes.data, 0, B, M)
    assert hra.lib.hrx_lookup_counts_host(cfg._ctx, 0, *args, 0, B, out.ctypes.data, None) == hra.HRX_OK and np.array_equal(out, counts)
    # refused calls write nothing
    out[:] = 0x5A5A5A5A
    mo = np.full(B, 0x5A5A5A5A, np.uint32)
    f = hra.lib.hrx_lookup_counts_host
    assert f(None, 0, *args, 0, B, out.ctypes.data, mo.ctypes.data) == hra.HRX_ERR_ARG
    assert f(cfg._ctx, 4, *args, 0, B, out.ctypes.data, mo.ctypes.data) == hra.HRX_ERR_ARG
    assert f(cfg._ctx, 0, *args, 0, B, out.ctypes.data + 4, mo.ctypes.data) == hra.HRX_ERR_ARG                  # counts not 16-byte aligned
    assert f(cfg._ctx, 0, *args, 1, B, out.ctypes.data, mo.ctypes.data) == hra.HRX_ERR_ARG                      # window past the batch
    assert f(cfg._ctx, 0, *args[:4], M - 1, *args[5:], 0, B, out.ctypes.data, mo.ctypes.data) == hra.HRX_ERR_ARG  # pitch < M
    assert f(cfg._ctx, 0, *args[:6], (1 << 24) + 1, 0, B, out.ctypes.data, mo.ctypes.data) == hra.HRX_ERR_ARG
    assert f(cfg._ctx, 0, *args[:3], None, *args[4:], 0, B, out.ctypes.data, mo.ctypes.data) == hra.HRX_ERR_ARG
    assert f(cfg._ctx, 0, *args, 0, B, None, mo.ctypes.data) == hra.HRX_ERR_ARG
    assert (out == 0x5A5A5A5A).all() and (mo == 0x5A5A5A5A).all()
    # the device forms on a host-only context: no device
    assert hra.lib.hrx_lookup_counts_device(cfg._ctx, 0, 16, 16, 16, 16, 0, B, M, 0, B, 16, 16, None) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_lookup_counts_device(None, 0, 16, 16, 16, 16, 0, B, M, 0, B, 16, 16, None) == hra.HRX_ERR_ARG
    # a clone counts with an image of its own; the planner's report
    c3, m3 = cfg.clone().lookup_counts_host(chars, lens, rec)
    assert np.array_equal(c3, counts) and np.array_equal(m3, misses)
    g, p = cfg.lookup_group(65536)
    assert p == 1 and g >= 2 and g & (g - 1) == 0 and g * W * 4 <= 64 * 1024 and cfg.lookup_group(1) == (1, 1)


def test_the_synthetic_256_state_dfa_needs_passes():
    a_txt, sub_txt = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=200)
    cfg = hra.RegexVerifyConfig.configure(64, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub_txt)])], device=hra.HRX_DEVICE_NONE)
    assert cfg.lookup_layout()[0]["trans"].stop == 65537 and cfg.lookup_words() * 4 > 160 * 1024
    assert cfg.lookup_group(65536) == (1, 2) and cfg.lookup_group(3) == (1, 2)
    chars, lens = synth.noise(4, 64, seed=1, alphabet=np.arange(256, dtype=np.uint8))
    lens[1] = 0
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    assert not misses.any() and counts[1, 0] == 64 and (counts[:, :65537].sum(1) == [63, 64, 63, 63]).all()


def test_permuted_lookup_columns_on_real_counts():
    M = 64
    cfg = _cfg(CFG_A, M)
    chars, lens = synth.ragged(12, M, seed=4)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    n_rows = 4096
    for b in range(12):
        for d, lay in enumerate(cfg.lookup_layout()):
            for name in ("trans", "start", "end"):
                m = counts[b][lay[name]]
                T = len(m)
                A, S = hra.permuted_lookup_columns(T, m, n_rows)
                assert len(A) == len(S) == n_rows and (np.diff(A) >= 0).all()
                want = m.astype(np.int64).copy()
                want[0] += n_rows - want.sum()
                assert np.array_equal(np.bincount(A, minlength=T), want)
                padded = np.bincount(S, minlength=T)
                assert padded[0] == 1 + n_rows - T and (padded[1:] == 1).all()
                assert ((A == S) | (A == np.concatenate([[-1], A[:-1]]))).all()
    m = counts[0][cfg.lookup_layout()[0]["start"]]
    with pytest.raises(ValueError):
        hra.permuted_lookup_columns(len(m), m, int(m.sum()) - 1)
    with pytest.raises(ValueError):
        hra.permuted_lookup_columns(3000, np.zeros(3000, np.uint32), 2999)
    A, S = hra.permuted_lookup_columns(3, [0, 2, 1], 3)             # no padding at all: row 0 is never looked up
    assert A.tolist() == [1, 1, 2] and sorted(S.tolist()) == [0, 1, 2] and S[0] == 1 and S[2] == 2


def test_the_stages_agree_on_the_run_layout():
    """counts, compress and permute read one layout of a string's run (csrc/hrx_lookup_run.hpp): two host-only contexts alive at once — one def, two defs —
    used alternately; the layout's slices tile the unpadded run in the order trans, start, end with load()'s row counts, the compressed table has
    lookup_words() cells per run and zero cells at the pad words alone, and every index lookup_permute_host gives lies in its lookup's slice"""
    M = 16
    cfgs = [_cfg(CFG_1, M), _cfg(CFG_23, M)]
    chars, lens = small_batch(M)
    pick = [2, 4, 6]                                        # n = 1, M - 1, M
    chars, lens = np.ascontiguousarray(chars[pick]), lens[pick]
    assert lens.tolist() == [1, M - 1, M]
    theta = np.array([7, 0, 0, 0], np.uint64)               # canonical: the cell of (a0, a1, a2, a3) is the integer 343 a0 + 49 a1 + 7 a2 + a3
    lays, counts, used = {}, {}, {}
    for step in ("layout", "table", "counts", "permute"):
        for i, cfg in enumerate(cfgs):
            W = cfg.lookup_words()
            if step == "layout":
                lay, rows, at = cfg.lookup_layout(), cfg.load(), 0
                assert W % 4 == 0 and len(lay) == cfg.num_defs == len(rows)
                for d in range(cfg.num_defs):
                    for name, n in (("trans", len(rows[d][0])), ("start", len(rows[d][1])), ("end", len(rows[d][1]))):
                        assert lay[d][name] == slice(at, at + n), (i, d, name)
                        at += n
                assert at <= W < at + 4
                lays[i], used[i] = lay, at
            elif step == "table":
                cells = cfg.lookup_compress_table_host(theta, canonical=True)
                assert cells.shape == (1, W, 4)
                zero = ~cells[0].any(axis=1)
                assert not zero[:used[i]].any() and zero[used[i]:].all()
            elif step == "counts":
                rec, msk, st = cfg.witness_batch_host(chars, lens)
                counts[i], misses = cfg.lookup_counts_host(chars, lens, rec)
                assert counts[i].shape == (3, W) and not counts[i][:, used[i]:].any()
            else:
                n_rows = max(sl.stop - sl.start for lay in lays[i] for sl in lay.values()) + 1
                res = cfg.lookup_permute_host(counts[i], n_rows)
                assert not res["overflow"].any()
                for d, lay in enumerate(lays[i]):
                    for k, name in enumerate(("trans", "start", "end")):
                        for key in ("a_idx", "s_idx"):
                            v = res[key][3 * d + k, :, :n_rows]
                            assert (v >= lay[name].start).all() and (v < lay[name].stop).all(), (i, d, name, key)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_lookup_host.cpp: csrc/hrx_lookup.hpp + csrc/hrx_lookup_host.cpp compiled into a program of their own with the address and
    undefined-behaviour sanitizers — hand-made rows, every image of them, values outside every table with the image a heap block of its exact size"""
    exe = str(tmp_path / "hrx_test_lookup_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_lookup_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "lookup host: ok" in out.stdout, out.stdout + out.stderr
