"""The tamper catalogue of tests/verify_cases.py is what it claims, on the host (no device): the rows come from witness_batch_host on a host-only context, the
words from hrx_verify_rows_host, the bits from the torch checker (tests/mock_prover.py), and the catalogue's a-priori table — written from include/hrx.h and
src/lib.rs, not from either checker — must hold against both for every entry.  tests/test_verify_tamper_gpu.py takes expected() from here and runs the same
catalogue through every form of verify_rows_kernel."""
import functools

import numpy as np
import pytest
import torch

import halo2_regex_amd as hra
import verify_cases as vc
from mock_prover import IntegerMockProver, FAIL_ACCEPT, FAIL_ENABLE

LOW = np.uint64(0xffffffff)
ALL_BUT_ENABLE = 511 & ~FAIL_ENABLE


def defs_of_text(defs_t):
    return [hra.RegexDefs(hra.AllstrRegexDef(t[0]), [hra.SubstrRegexDef(s) for s in t[1]]) for t in defs_t]


def torch_words(cfg, chars, lens, rec, msk):
    """IntegerMockProver.verify over numpy string-major rows: (B,) int64 of FAIL_* bits"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view({np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype, a.dtype)))
    return IntegerMockProver.from_config(cfg).verify(t(chars), torch.from_numpy(np.asarray(lens).astype(np.int64)), t(rec), t(msk), cfg.max_chars_size).numpy()


class Expected:
    """one def set's catalogue on the host: the clean rows and words, the rows with every mutation applied, the host twin's words and the torch checker's bits of those,
    and the class of every entry with the `open` ones decided by the torch checker"""

    def __init__(self, name):
        self.cat = cat = vc.Catalogue(name)
        cfg = hra.RegexVerifyConfig.configure(cat.M, defs_of_text(cat.defs_t), device=hra.HRX_DEVICE_NONE)
        self.rec, self.msk, self.st = cfg.witness_batch_host(cat.chars, cat.lens)
        self.clean = cfg.verify_rows_host(cat.chars, cat.lens, self.rec, self.msk)
        self.clean_bits = torch_words(cfg, cat.chars, cat.lens, self.rec, self.msk)
        self.rec_mut, self.msk_mut, self.chars_mut = cat.apply(self.rec, self.msk, cat.chars)
        self.want = cfg.verify_rows_host(self.chars_mut, cat.lens, self.rec_mut, self.msk_mut)
        self.bits = torch_words(cfg, self.chars_mut, cat.lens, self.rec_mut, self.msk_mut)
        self.cls = [c if c != "open" else ("must_fail" if self.bits[m[0]] != self.clean_bits[m[0]] else "must_not_matter") for c, m in zip(cat.cls, cat.muts)]


@functools.lru_cache(maxsize=None)
def expected(name):
    return Expected(name)


def check_classes(cat, cls, words, clean, tag=""):
    """every catalogue entry against verdict words (B,) uint64: must_fail — nonzero, the guaranteed bit, bits 57 .. 63 clear, the row field as the table gives it;
    must_not_matter and the fillers — the clean word.  Returns the union of the check bits of the must_fail strings."""
    seen = 0
    for (b, kind, r, d, _), c, bit, row in zip(cat.muts, cls, cat.bit, cat.row):
        v, v0 = int(words[b]), int(clean[b])
        what = "%s%s string %d %s row %d def %d (n = %d): %s, clean %s" % (tag, cat.name, b, kind, r, d, cat.lens[b], hra.explain_verdict(v), hra.explain_verdict(v0))
        if c == "must_not_matter":
            assert v == v0, what
            continue
        assert v != 0 and v & bit == bit and v >> 57 == 0, what
        got_row = v >> 32
        if row is not None and row[0] == "eq":
            assert got_row == (min(row[1], v0 >> 32) if v0 else row[1]), what
        elif row is not None:
            assert got_row <= row[1], what
        seen |= v & 0xffffffff
    for b in cat.fillers:
        assert words[b] == clean[b], "%s%s: filler string %d changed" % (tag, cat.name, b)
    return seen


@pytest.mark.parametrize("name", list(vc.SETS))
def test_base_strings_are_clean_and_reveal_their_ranges(name):
    """every base string: status 0; the word is 0 in the one-def sets and where n == M, exactly the accept chain at row n in the others (def 0 ends outside its accepted
    state); the host twin and the torch checker agree; the masked rows are non-zero on exactly the rows of the confirmed ranges, one of them across row 31 / 32 and one
    across the last 16-row border below n; the big set's walk leaves the first 64 states"""
    e = expected(name)
    cat = e.cat
    assert cat.M == 139 and cat.B == len(cat.muts) + len(cat.fillers) and set(cat.lens.tolist()) == {64, 101, 139} and (cat.lens >= 2).all()
    assert (e.st & np.uint64(0xff) == 0).all()
    for b in range(cat.B):
        n = int(cat.lens[b])
        want = 0 if cat.D == 1 or n == cat.M else FAIL_ACCEPT | n << 32
        assert int(e.clean[b]) == want and int(e.clean_bits[b]) == want & 0xffffffff, (name, b, hra.explain_verdict(e.clean[b]))
    for f in cat.fillers:
        n = int(cat.lens[f])
        rows = set()
        for k, a, b in cat.ranges[n]:
            rows |= set(range(a, b + 1))
        assert set(np.nonzero(e.msk[f])[0].tolist()) == rows, (name, n)
        assert sorted({k for k, _, _ in cat.ranges[n]}) == list(range(cat.D))
        assert any(a <= 31 and b >= 32 for _, a, b in cat.ranges[n]) and any(a < 16 * ((n - 2) // 16) <= b for _, a, b in cat.ranges[n])
    if name == "big":
        assert cat.defs_t[0][0].splitlines()[2] == "303" and int((e.rec[..., 0] & 0xffff).max()) > 64
    if name == "second":
        assert int(((e.rec[..., 0] >> 16) & 0xff).max()) == 2


@pytest.mark.parametrize("name", list(vc.SETS))
def test_catalogue_against_both_checkers(name):
    """after the mutations: the host twin's bits are the torch checker's on every string; every entry's class, guaranteed bit and row field hold; every cell was changed;
    over the set every check bit but the enable gate is seen (enable is derived from n: its gate cannot fire); every (kind, row) has a must_fail entry in some length
    class — but three input bytes that no class can make matter: (char, M - 1), a row that is disabled below n == M and whose transition lookup with n == M reads
    the cell nobody assigns, and (char, 101), (char, 102), which are edge rows of the class n = 101 alone, as its rows n and n + 1"""
    e = expected(name)
    cat = e.cat
    b, r, d, _, _ = cat.cells("rec")
    assert (e.rec_mut[b, r, d] != e.rec[b, r, d]).all() and (e.rec_mut != e.rec).sum() == len(b)
    b, r, d, _, _ = cat.cells("msk")
    assert (e.msk_mut[b, r] != e.msk[b, r]).all() and (e.msk_mut != e.msk).sum() == len(b)
    b, r, d, _, _ = cat.cells("chr")
    assert (e.chars_mut[b, r] != cat.chars[b, r]).all() and (e.chars_mut != cat.chars).sum() == len(b)
    assert len({m[0] for m in cat.muts}) == len(cat.muts)                  # one mutation per string
    assert np.array_equal((e.want & LOW).astype(np.int64), e.bits), "%s: string %d" % (name, np.nonzero((e.want & LOW).astype(np.int64) != e.bits)[0][0])
    seen = check_classes(cat, e.cls, e.want, e.clean)
    assert seen == ALL_BUT_ENABLE, "checks never seen: %s" % hra.explain_verdict(ALL_BUT_ENABLE & ~seen)
    pairs = {(m[1], m[2]) for m in cat.muts}
    failing = {(m[1], m[2]) for m, c in zip(cat.muts, e.cls) if c == "must_fail"}
    assert pairs - failing == {("char", 101), ("char", 102), ("char", cat.M - 1)}      # (rows 101 and 102 are edge rows of the class n = 101 alone: n and n + 1)
    assert {(m[1], m[2]) for m in cat.muts if m[2] in (31, 32, 33)} >= {(k, r) for k in vc.OPS for r in (31, 32, 33)}
    c = cat.counts()
    assert c["open"] == 2 * cat.D and c["must_fail"] + c["must_not_matter"] + c["open"] == len(cat.muts)


def test_poison_kinds_are_listed():
    cat = expected("one").cat
    assert cat.poison == [("tail_rec", "must_not_matter"), ("tail_msk", "must_not_matter"), ("gap", "must_not_matter")]
    assert vc.edge_rows(139, 139) == [0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 137, 138]
    assert vc.edge_rows(64, 139) == [0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 137, 138]


def test_counts(capsys):
    """the catalogue's size per def set (printed: pytest -s)"""
    for name in vc.SETS:
        e = expected(name)
        seen = 0
        for m, c in zip(e.cat.muts, e.cls):
            seen |= int(e.bits[m[0]]) if c == "must_fail" else 0
        n = {c: e.cls.count(c) for c in ("must_fail", "must_not_matter")}
        print("%-7s D %d  strings %5d  must_fail %5d  must_not_matter %3d (of them decided by the torch checker: %d fail, %d do not)  bits 0x%03x" % (
            name, e.cat.D, e.cat.B, n["must_fail"], n["must_not_matter"], sum(1 for a, b in zip(e.cat.cls, e.cls) if a == "open" and b == "must_fail"),
            sum(1 for a, b in zip(e.cat.cls, e.cls) if a == "open" and b == "must_not_matter"), seen))
        assert n["must_fail"] > 20 * len(vc.OPS)
