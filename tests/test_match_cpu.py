"""Match-only entry points (include/hrx.h MATCH: hrx_match_batch_host, hrx_describe_match) on host-only contexts: status bit for bit
what the witness path computes, revealed runs = the run-length encoding of the oracle's masked_substr_id column, the reference's own
expected substrings, truncation at max_spans, and which device kernel the planner names per config."""
import os

import numpy as np
import pytest

import carry_defs as cd
import fuzz_defs as fd
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import OracleDefs, DFA_DIR, reference_cases

CFG_1 = [["regex1_test_lookup.txt", ["substr1_test_lookup.txt"]]]
CFG_A = [["regex1_test_lookup.txt", ["substr1_test_lookup.txt"]], ["regex2_test_lookup.txt", ["substr2_test_lookup.txt"]]]
CFG_3 = [["regex3_test_lookup.txt", ["substr3_test_lookup.txt"]]]
CFG_23 = [["regex2_test_lookup.txt", ["substr2_test_lookup.txt"]], ["regex3_test_lookup.txt", ["substr3_test_lookup.txt"]]]
HDR = lambda n, ns: [n + "_lookup.txt", ["%s_substr%d.txt" % (n, k) for k in range(ns)]]
CFG_H3 = [HDR("header_from", 1), HDR("header_to", 1), HDR("header_subject", 3)]
CFG_H4 = CFG_H3 + CFG_1


def _defs(names):
    return [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(os.path.join(DFA_DIR, a)),
                          [hra.SubstrRegexDef.read_from_text(os.path.join(DFA_DIR, s)) for s in subs]) for a, subs in names]


def _cfg(names, M, device=hra.HRX_DEVICE_NONE):
    return hra.RegexVerifyConfig.configure(M, _defs(names), device=device)


def rle_masked(masked, lens, status):
    """Expected (counts, runs) from masked rows (B, M) u16: maximal runs of one non-zero masked_substr_id (masked >> 8) below n,
    as (substr_id, start, length); no runs where the status code != 0."""
    counts, runs = [], []
    for b in range(masked.shape[0]):
        r = []
        if not int(status[b]) & 0xff:
            v = masked[b].astype(np.int64) >> 8
            v[int(lens[b]):] = 0
            cuts = np.flatnonzero(np.diff(v)) + 1                      # where the value changes
            starts = np.concatenate(([0], cuts))
            ends = np.concatenate((cuts, [len(v)]))
            r = [(int(v[s]), int(s), int(e - s)) for s, e in zip(starts, ends) if v[s] != 0]
        counts.append(len(r))
        runs.append(r)
    return counts, runs


def check_match(oracle, names, chars, lens, M, max_spans=64, cfg=None, o=None):
    cfg = cfg or _cfg(names, M)
    o = o or OracleDefs.from_files(oracle, names)
    _, omsk, ost = o.witness_batch(chars, lens, M, threads=8)
    st, cnt, sp = cfg.match_batch_host(chars, lens, max_spans=max_spans)
    assert np.array_equal(st, ost)
    ecnt, eruns = rle_masked(omsk, lens, ost)
    assert cnt.tolist() == ecnt
    got = hra.decode_spans(cnt, sp)
    for b in range(len(lens)):
        assert got[b] == eruns[b][:max_spans], b
    return st, cnt, sp


@pytest.mark.parametrize("case", [c for c in reference_cases() if c["masked_outputs_asserted"]],
                         ids=[c["name"] for c in reference_cases() if c["masked_outputs_asserted"]])
def test_reference_expected_substrs(oracle, case):
    """lib.rs:1046-1058: the revealed substrings are the test's expected_substrs, ids 1, 2, ... in list order."""
    M = case["max_chars_size"]
    inp = case["input"].encode("latin-1")
    stride = max(16, -(-max(len(inp), 1) // 16) * 16)
    chars = np.zeros((1, stride), np.uint8)
    chars[0, :len(inp)] = np.frombuffer(inp, np.uint8)
    lens = np.array([len(inp)], np.uint32)
    cfg = _cfg(case["defs"], M)
    st, cnt, sp = check_match(oracle, case["defs"], chars, lens, M, cfg=cfg)
    got = hra.revealed_substrings(chars, lens, st, cnt, sp)[0]
    want = [(k + 1, start, text.encode("latin-1")) for k, (start, text) in enumerate(case["expected_substrs"])]
    assert got == want


@pytest.mark.parametrize("M", [1, 7, 63, 64, 65, 1024])
@pytest.mark.parametrize("names", [CFG_1, CFG_A, CFG_23], ids=["regex1", "regex12", "regex23"])
def test_ragged_lengths(oracle, names, M):
    rng = np.random.default_rng(M)
    B = 96
    stride = -(-(M + 1) // 16) * 16
    chars, _ = synth.regex1_planted(B, M, seed=M, stride=stride) if M >= 16 else synth.noise(B, M, seed=M, stride=stride)
    lens = rng.integers(0, M + 1, B).astype(np.uint32)
    lens[0], lens[1] = 0, M
    lens[2] = M + 1           # n > M: status 3, count 0
    check_match(oracle, names, chars, lens, M)


@pytest.mark.parametrize("seed", [7, 8, 9])
def test_reveal_stress(oracle, seed):
    M = 1024
    chars, lens = synth.reveal_stress(256, M, seed=seed)
    check_match(oracle, CFG_A, chars, lens, M)
    check_match(oracle, CFG_3, chars, lens, M)


def _regex1_hit(name):
    """a string regex1 accepts whose one revealed substring is `name` (substr1: the bytes after '@' up to '.')"""
    return b"email was meant for @" + name + b"."


@pytest.mark.parametrize("tiles", [3, 30, 300])
def test_long_spans_and_one_that_never_closes(oracle, tiles):
    """runs that close `tiles` tiles after they open, and one whose string ends inside it.  On regex1 every row of a run carries an end flag (the substring's end
    state is its loop state), so the unterminated match is revealed like the others: all of these optimistic end masks are CONFIRMED that much later, none is
    fixed.  The lever strings of tests/carry_defs.py behind them are the ones that are taken back, over the same number of tiles: by a second start, by the string's
    end, by reaching M, with islands of tagged rows inside (the run emitter rolls back), next to a confirmed one."""
    M = 64 * (tiles + 2)
    stride = -(-(M + 1) // 16) * 16
    B = 4
    chars = np.zeros((B, stride), np.uint8)
    lens = np.zeros(B, np.uint32)
    body = b"x" * (64 * tiles)
    texts = [_regex1_hit(body), b"email was meant for @" + body, b"prefix " + _regex1_hit(body[:-10]) + b" tail", _regex1_hit(b"y")]
    for b, t in enumerate(texts):
        t = t[:M]
        chars[b, :len(t)] = np.frombuffer(t, np.uint8)
        lens[b] = len(t)
    check_match(oracle, CFG_1, chars, lens, M)
    check_match(oracle, CFG_A, chars, lens, M)
    a, b = 21, 21 + 64 * tiles
    made = [cd.sc_second_start(M, a, b), cd.sc_string_end(M, a, b), cd.sc_reach_m(M, a), cd.sc_islands(M, a, b, confirmed=False), cd.sc_confirmed(M, a, b),
            cd.sc_second_start(M, 0, b), cd.sc_end_at_last_row(M, a)]
    lever = cd.lever_defs(1)
    chars = np.zeros((len(made), stride), np.uint8)
    lens = np.array([len(v) for v, _, _ in made], np.uint32)
    for k, (v, code, ranges) in enumerate(made):
        chars[k, :len(v)] = v
    o = OracleDefs(oracle, [(t, subs) for t, subs, _ in lever])
    _, omsk, ost = o.witness_batch(chars, lens, M)
    assert not (ost & np.uint64(0xff)).any()
    for k, (v, code, ranges) in enumerate(made):      # they are what they say: taken back means nothing of the range is revealed
        for r0, r1, kind in ranges:
            assert omsk[k, r0:min(r1, M)].all() if kind == "confirmed" else not omsk[k, r0:min(r1, M)].any(), (k, kind)
    cfg = hra.RegexVerifyConfig.configure(M, [hra.RegexDefs(hra.AllstrRegexDef(t), [hra.SubstrRegexDef(x) for x in subs]) for t, subs, _ in lever], device=hra.HRX_DEVICE_NONE)
    check_match(oracle, None, chars, lens, M, cfg=cfg, o=o)


def test_sid_changes_without_flags_and_overlap(oracle):
    """two defs whose substrings abut or overlap (SID changes inside a pending range without a start / end flag; status 2 where two
    defs flag one row) and invalid transitions (status 1, count 0)"""
    M = 256
    texts = [b"email was meant for @y. Also for x.", b"@ab.c.x.", b"email was meant for @yx.", b"\x00\x01\xff@y.x.",
             b"email was meant for @y.x", b"x." * 100]
    chars = np.zeros((len(texts), 272), np.uint8)
    lens = np.zeros(len(texts), np.uint32)
    for b, t in enumerate(texts):
        chars[b, :len(t)] = np.frombuffer(t, np.uint8)
        lens[b] = len(t)
    for names in (CFG_A, CFG_23, CFG_1 + CFG_3):
        check_match(oracle, names, chars, lens, M)


def test_truncation_and_status_only(oracle):
    M = 1024
    chars, lens = synth.reveal_stress(64, M, seed=11)
    o = OracleDefs.from_files(oracle, CFG_A)
    _, omsk, ost = o.witness_batch(chars, lens, M)
    ecnt, eruns = rle_masked(omsk, lens, ost)
    assert max(ecnt) > 2
    cfg = _cfg(CFG_A, M)
    st, cnt, sp = cfg.match_batch_host(chars, lens, max_spans=2)
    assert np.array_equal(st, ost) and cnt.tolist() == ecnt          # exact counts past max_spans
    got = hra.decode_spans(cnt, sp)
    assert all(got[b] == eruns[b][:2] for b in range(len(lens)))
    st0, cnt0, sp0 = cfg.match_batch_host(chars, lens, max_spans=0)    # status only
    assert np.array_equal(st0, ost) and cnt0.tolist() == ecnt and sp0.shape == (64, 0)
    with pytest.raises(hra.HrxError):
        cfg.match_batch_host(chars, lens, max_spans=(1 << 16) + 1)


@pytest.mark.parametrize("seed", list(range(0, 24)))
def test_fuzz_defs(oracle, seed):
    """1 .. 7 defs of tests/fuzz_defs.py (partial DFAs, odd M, undefined transitions at tile borders, every byte value)"""
    case = fd.make_case(seed, fd.Shape(1, 7, "small", "any"))
    defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
    cfg = hra.RegexVerifyConfig.configure(case.M, defs, device=hra.HRX_DEVICE_NONE)
    o = OracleDefs(oracle, [(a.encode(), [t.encode() for t in subs]) for a, subs, _ in case.defs_t])
    _, omsk, ost = o.witness_batch(case.chars, case.lens, case.M)
    st, cnt, sp = cfg.match_batch_host(case.chars, case.lens, max_spans=8)
    rec, msk, wst = cfg.witness_batch_host(case.chars, case.lens)
    assert np.array_equal(st, wst) and np.array_equal(st, ost)
    ecnt, eruns = rle_masked(omsk, case.lens, ost)
    assert cnt.tolist() == ecnt
    got = hra.decode_spans(cnt, sp)
    assert all(got[b] == eruns[b][:8] for b in range(case.B))


def test_describe_match_pins_the_path():
    """fused where the planner walks one lane per string on the narrow LDS table, via rows elsewhere"""
    def desc(names, B, M, layout=0):
        return _cfg(names, M).describe_match(B, layout=layout)
    assert desc(CFG_1, 65536, 1024).startswith("hrx::match_lane_kernel<1, false, false> grid=256 threads=256 ")           # configs[1], the headline
    assert desc(CFG_23, 262144, 2048, 2).startswith("hrx::match_lane_kernel<2, false, false> ")              # configs[2]'s regex2+3 share
    assert desc(CFG_H3, 32768, 32768).startswith("hrx::match_lane_kernel<3, false, false> grid=256 threads=128 ")                # configs[3] share
    d4 = desc(CFG_H4, 65536, 2048)
    assert d4.startswith("via rows") and "spans_from_masked_pm_kernel" in d4 and "witness_pmd_kernel<4" in d4
    d5 = desc(CFG_H4 + CFG_23[:1], 4096, 1024)
    assert d5.startswith("via rows") and "witness_pmd_kernel<5" in d5
    long = desc(CFG_1, 8192, 32768)                                                            # few long strings: the chunked witness
    assert long.startswith("via rows") and "chunked" in long
    a_txt, sub = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=40)
    big = hra.RegexVerifyConfig.configure(4096, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub)])], device=hra.HRX_DEVICE_NONE)
    assert big.describe_match(131072).startswith("hrx::match_lane_kernel<1, false, true> ")    # configs[4]: the 256 KiB narrow table does not fit LDS, the HALF one does
    def forced(names, flags, M=1024):
        os.environ["HRX_DEBUG_FLAGS"] = str(flags)
        try:
            return _cfg(names, M)
        finally:
            os.environ.pop("HRX_DEBUG_FLAGS", None)
    assert forced(CFG_1, 1 << 32).describe_match(65536).startswith("via rows")
    for names in (CFG_1, CFG_23, CFG_H3):
        D = len(names)
        for flags, args in ((0x80000, "false, false"), (0x200000, "false, false"), (0x400000, "false, true"), (0x2000, "false, true"), (0x40000, "true, false")):
            assert forced(names, flags).describe_match(65536).startswith("hrx::match_lane_kernel<%d, %s> " % (D, args)), (D, flags)


def test_runs_from_masked_helper():
    masked = np.array([[0, 0x141, 0x142, 0x241, 0x241, 0, 0x141, 0x141]], np.uint16)
    counts, runs = rle_masked(masked, np.array([7], np.uint32), np.zeros(1, np.uint64))
    assert (counts, runs) == ([3], [[(1, 1, 2), (2, 3, 2), (1, 6, 1)]])
    assert hra.runs_from_masked(masked, np.array([7], np.uint32), np.zeros(1, np.uint64)) == (counts, runs)


def test_via_rows_scratch_bound():
    """one string's witness rows larger than the via-rows scratch: an error, not an allocation past the header's bound"""
    cfg = _cfg(CFG_H4 * 3, 1 << 24)
    with pytest.raises(hra.HrxError):
        cfg.describe_match(16)
    assert _cfg(CFG_H4 * 3, 1 << 20).describe_match(16).startswith("via rows")
