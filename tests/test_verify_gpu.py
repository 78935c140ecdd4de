"""VERIFY on the device (hrx_verify_rows_device / _planes, verify_rows_kernel of csrc/hrx_kernel_verify.hip).  The rows come from the device witness entry
points; the yardsticks are the host twin (hrx_verify_rows_host over the same rows copied to the host) for the whole verdict word and the torch checker
(tests/mock_prover.py) for its check bits — neither is the kernel under test.

  clean rows, every form     seven def sets x string-major tight / pitched, position-major from both input layouts, record planes, row stripes
  block border               65536 + 300 strings x 19 rows, clean, then one masked cell and one record of string 65536 + 5 changed on the device
  tamper matrix              one mutation per string on the device copy of the rows, every check bit but the enable gate, at tile-edge rows
  long ranges                lever definitions, 2048 rows: a range of M - 2 rows confirmed by an end-only event, ranges taken back three ways
  contract                   lens > M, first call inside a capture, capture and replay, refused calls, a host-only context

Every verdict buffer lies between two poisoned 4-KiB guards."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import carry_defs as cd
import fr_cases as fc
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from mock_prover import IntegerMockProver, FAIL_ACCEPT, FAIL_ENABLE, FAIL_MASK
from oracle_lib import DFA_DIR
from test_match_cpu import CFG_H4

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CFG_1 = [["regex1_test_lookup.txt", ["substr1_test_lookup.txt"]]]
CFG_A = CFG_1 + [["regex2_test_lookup.txt", ["substr2_test_lookup.txt"]]]
CFG_123 = CFG_A + [["regex3_test_lookup.txt", ["substr3_test_lookup.txt"]]]
POISON = 0x5A5A5A5A5A5A5A5A
GUARD = 512                   # u64 words: 4 KiB before and behind the verdicts
ALL_BUT_ENABLE = 511 & ~FAIL_ENABLE
PM, PM_IN = hra.LAYOUT_POSITION_MAJOR, hra.LAYOUT_POSITION_MAJOR | hra.LAYOUT_INPUT_POSITION_MAJOR


def defs_of_files(names):
    return [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(os.path.join(DFA_DIR, a)), [hra.SubstrRegexDef.read_from_text(os.path.join(DFA_DIR, s)) for s in subs])
            for a, subs in names]


def defs_of_text(defs_t):
    return [hra.RegexDefs(hra.AllstrRegexDef(t[0]), [hra.SubstrRegexDef(s) for s in t[1]]) for t in defs_t]


def guarded(B):
    raw = torch.full((GUARD + B + GUARD,), POISON, dtype=torch.int64, device=DEV)
    return raw, raw[GUARD:GUARD + B]


def guards_intact(raw, B):
    return bool((raw[:GUARD] == POISON).all()) and bool((raw[GUARD + B:] == POISON).all())


class Rows:
    """the witness rows of one batch on the device in one form: sm, sm-pitched, pm, planes (one def: the two row stripes); "-in": position-major input"""

    def __init__(self, cfg, form, chars, lens):
        self.cfg, self.form, self.B, self.M, self.D, self.stride = cfg, form, len(lens), cfg.max_chars_size, cfg.num_defs, chars.shape[1]
        self.chars, self.lens = chars, np.asarray(lens, np.uint32)
        self.d_lens = torch.from_numpy(self.lens.astype(np.int32)).to(DEV)
        d_chars = torch.from_numpy(chars).to(DEV)
        in_pm = form.endswith("-in")
        base = form[:-3] if in_pm else form
        self.src, self.kw = (hra.chars_to_position_major(d_chars), dict(chars_pm_stride=self.stride)) if in_pm else (d_chars, {})
        self.planes = None
        if base in ("sm", "sm-pitched"):
            self.layout = hra.LAYOUT_STRING_MAJOR
            self.rec, self.msk, self.st = cfg.witness_batch(d_chars, self.d_lens, out=cfg.alloc_outputs(self.B, DEV, pitched=base == "sm-pitched"))
            assert base == "sm" or self.rec.stride(0) // self.D == hra.recommended_pitches(self.M)[0]
        elif base == "pm":
            self.layout = PM_IN if in_pm else PM
            self.rec, self.msk, self.st = cfg.witness_batch_position_major(self.src, self.d_lens, **self.kw)
        else:
            assert base == "planes"
            self.layout = PM_IN if in_pm else PM
            out = cfg.alloc_output_planes(self.B, DEV, stripes=2 if self.D == 1 else None)
            self.planes, self.msk, self.st = cfg.witness_batch_planes(self.src, self.d_lens, out=out, **self.kw)
            self.rec = None
        torch.cuda.synchronize()

    def verify(self, lens=None, out=None):
        """the device verdicts between their guards, as uint64"""
        raw, v = guarded(self.B)
        got = self.cfg.verify_rows(self.src, self.d_lens if lens is None else lens, self.rec, self.msk, layout=self.layout, planes=self.planes, out=v, **self.kw)
        torch.cuda.synchronize()
        assert got.data_ptr() == v.data_ptr() and guards_intact(raw, self.B), self.form + ": a guard of the verdicts was written"
        return v.cpu().numpy().view(np.uint64)

    def host_rows(self):
        """the rows as they lie on the device now, copied out and turned string-major: (B, M, D) uint32, (B, M) uint16"""
        B, M, D = self.B, self.M, self.D
        msk = self.msk.cpu().numpy().view(np.uint16)
        if self.layout == hra.LAYOUT_STRING_MAJOR:
            return self.rec.cpu().numpy().view(np.uint32), msk
        if self.planes is not None:
            rec, msk = hra.planes_to_string_major([p.cpu().numpy().view(np.uint32) for p in self.planes], msk, B, M, D)
        else:
            rec, msk = hra.position_major_to_string_major(self.rec.cpu().numpy().view(np.uint32), msk, B, M, D)
        return np.ascontiguousarray(rec), np.ascontiguousarray(msk)

    def host_words(self, lens=None):
        rec, msk = self.host_rows()
        return self.cfg.verify_rows_host(self.chars, self.lens if lens is None else lens, rec, msk)

    # one cell of the device copy: (tensor, flat index)
    def _rec_cell(self, b, r, d):
        B, M, D = self.B, self.M, self.D
        if self.layout == hra.LAYOUT_STRING_MAJOR:
            return self.rec, (b, r, d)
        k, bl = b // hra.PM_BLOCK, b % hra.PM_BLOCK
        nb, q4 = min(hra.PM_BLOCK, B - k * hra.PM_BLOCK), (M + 3) // 4
        if self.planes is None:
            return self.rec, k * hra.PM_BLOCK * q4 * D * 4 + ((r // 4 * D + d) * nb + bl) * 4 + r % 4
        R = len(self.planes) // D
        q, slots = r // 4, (q4 + R - 1) // R
        return self.planes[(q % R) * D + d], k * hra.PM_BLOCK * slots * 4 + ((q // R) * nb + bl) * 4 + r % 4

    def _msk_cell(self, b, r):
        if self.layout == hra.LAYOUT_STRING_MAJOR:
            return self.msk, (b, r)
        k, bl = b // hra.PM_BLOCK, b % hra.PM_BLOCK
        nb, q8 = min(hra.PM_BLOCK, self.B - k * hra.PM_BLOCK), (self.M + 7) // 8
        return self.msk, k * hra.PM_BLOCK * q8 * 8 + (r // 8 * nb + bl) * 8 + r % 8

    def xor_rec(self, b, r, d, bits):
        t, i = self._rec_cell(b, r, d)
        t[i] = int(np.array([(int(t[i]) & 0xffffffff) ^ bits], np.uint32).view(np.int32)[0])

    def set_msk(self, b, r, value):
        t, i = self._msk_cell(b, r)
        t[i] = int(np.array([value & 0xffff], np.uint16).view(np.int16)[0])

    def get_msk(self, b, r):
        t, i = self._msk_cell(b, r)
        return int(t[i]) & 0xffff

    # many cells at once (numpy index arrays in, flat indices into a buffer's whole storage out): the rows behind M of a pitched string's slot and of a
    # position-major buffer's last quad / octet can be addressed too
    def rec_buffers(self):
        if self.planes is not None:
            return list(self.planes)
        return [self.rec.as_strided((self.B * self.rec.stride(0),), (1,))] if self.layout == hra.LAYOUT_STRING_MAJOR else [self.rec]

    def msk_buffer(self):
        return self.msk.as_strided((self.B * self.msk.stride(0),), (1,)) if self.layout == hra.LAYOUT_STRING_MAJOR else self.msk

    def chr_buffer(self):
        return self.src.view(-1)

    def _block(self, b):
        k = b // hra.PM_BLOCK
        return k, b % hra.PM_BLOCK, np.minimum(hra.PM_BLOCK, self.B - k * hra.PM_BLOCK)

    def rec_cells(self, b, r, d):
        """(number of the buffer of rec_buffers(), index into it) of the records (b, r, d)"""
        b, r, d = (np.asarray(a, np.int64) for a in (b, r, d))
        M, D = self.M, self.D
        if self.layout == hra.LAYOUT_STRING_MAJOR:
            return np.zeros(len(b), np.int64), (b * (self.rec.stride(0) // D) + r) * D + d
        (k, bl, nb), q4 = self._block(b), (M + 3) // 4
        if self.planes is None:
            return np.zeros(len(b), np.int64), k * hra.PM_BLOCK * q4 * D * 4 + ((r // 4 * D + d) * nb + bl) * 4 + r % 4
        R = len(self.planes) // D
        q, slots = r // 4, (q4 + R - 1) // R
        return (q % R) * D + d, k * hra.PM_BLOCK * slots * 4 + ((q // R) * nb + bl) * 4 + r % 4

    def msk_cells(self, b, r):
        b, r = np.asarray(b, np.int64), np.asarray(r, np.int64)
        if self.layout == hra.LAYOUT_STRING_MAJOR:
            return b * self.msk.stride(0) + r
        k, bl, nb = self._block(b)
        return k * hra.PM_BLOCK * ((self.M + 7) // 8) * 8 + (r // 8 * nb + bl) * 8 + r % 8

    def chr_cells(self, b, r):
        """input byte r of string b in the buffer verify reads: chunk r / 16 of a block of nb strings where the input is position-major"""
        b, r = np.asarray(b, np.int64), np.asarray(r, np.int64)
        if not self.layout & hra.LAYOUT_INPUT_POSITION_MAJOR:
            return b * self.stride + r
        k, bl, nb = self._block(b)
        return k * hra.PM_BLOCK * self.stride + ((r // 16) * nb + bl) * 16 + r % 16

    def update(self, bufs, which, idx, keep, flip):
        """buf[idx] = (buf[idx] & keep) ^ flip: per buffer one indexed read and one indexed write; every index is checked against the buffer's size here, on the host"""
        which, idx, keep, flip = (np.asarray(a, np.int64) for a in (which, idx, keep, flip))
        for j, t in enumerate(bufs):
            sel = np.nonzero(which == j)[0]
            if not len(sel):
                continue
            i = idx[sel]
            assert 0 <= i.min() and i.max() < t.numel() and len(np.unique(i)) == len(i), self.form
            u, s = {1: (np.uint8, np.uint8), 2: (np.uint16, np.int16), 4: (np.uint32, np.int32)}[t.element_size()]
            ti = torch.from_numpy(i).to(DEV)
            new = (t[ti].cpu().numpy().view(u) & keep[sel].astype(u)) ^ flip[sel].astype(u)
            t[ti] = torch.from_numpy(new.view(s)).to(DEV)
        torch.cuda.synchronize()

    def apply(self, cat):
        """every mutation of a verify_cases.Catalogue on the device copy, addressed as this form lays the cells out"""
        b, r, d, keep, flip = cat.cells("rec")
        which, idx = self.rec_cells(b, r, d)
        self.update(self.rec_buffers(), which, idx, keep, flip)
        b, r, d, keep, flip = cat.cells("msk")
        self.update([self.msk_buffer()], np.zeros(len(b)), self.msk_cells(b, r), keep, flip)
        b, r, d, keep, flip = cat.cells("chr")
        self.update([self.chr_buffer()], np.zeros(len(b)), self.chr_cells(b, r), keep, flip)

    def poison_unjudged(self, rec_value, msk_value, chr_value):
        """the cells verify must never judge, all strings at once: the rows M .. of the last quad (records, every def) and of the last octet (masked rows) of a
        position-major form, the rows M .. pitch - 1 of a pitched string's slot, the input bytes n .. stride - 1.  Returns how many cells of each kind there were."""
        B, M, D = self.B, self.M, self.D
        if self.layout == hra.LAYOUT_STRING_MAJOR:
            rec_end, msk_end = self.rec.stride(0) // D, self.msk.stride(0)
        else:
            rec_end, msk_end = (M + 3) // 4 * 4, (M + 7) // 8 * 8
        count = {}
        b, r, d = (a.reshape(-1) for a in np.meshgrid(np.arange(B), np.arange(M, rec_end), np.arange(D), indexing="ij"))
        count["rec"] = len(b)
        which, idx = self.rec_cells(b, r, d)
        self.update(self.rec_buffers(), which, idx, np.zeros(len(b)), np.full(len(b), rec_value))
        b, r = (a.reshape(-1) for a in np.meshgrid(np.arange(B), np.arange(M, msk_end), indexing="ij"))
        count["msk"] = len(b)
        self.update([self.msk_buffer()], np.zeros(len(b)), self.msk_cells(b, r), np.zeros(len(b)), np.full(len(b), msk_value))
        b, r = np.nonzero(np.arange(self.stride)[None, :] >= self.lens[:, None].astype(np.int64))
        count["chr"] = len(b)
        self.update([self.chr_buffer()], np.zeros(len(b)), self.chr_cells(b, r), np.zeros(len(b)), np.full(len(b), chr_value))
        return count

    def host_chars(self):
        """the input as verify reads it now, copied out and turned string-major: (B, stride) uint8"""
        c = self.src.cpu().numpy()
        if not self.layout & hra.LAYOUT_INPUT_POSITION_MAJOR:
            return c
        out = np.empty((self.B, self.stride), np.uint8)
        for k0 in range(0, self.B, hra.PM_BLOCK):
            nb = min(hra.PM_BLOCK, self.B - k0)
            out[k0:k0 + nb] = c[k0 * self.stride:(k0 + nb) * self.stride].reshape(self.stride // 16, nb, 16).transpose(1, 0, 2).reshape(nb, self.stride)
        return out


def torch_bits(cfg, rows, rec, msk):
    mp = IntegerMockProver.from_config(cfg)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view({np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype, a.dtype)))
    return mp.verify(t(rows.chars), torch.from_numpy(rows.lens.astype(np.int64)), t(rec), t(msk), rows.M).numpy()


def stress_batches(M):
    out = []
    for chars, lens in (synth.reveal_stress(300, 260, seed=5), synth.ragged(300, M, seed=7)):
        lens = lens.copy()
        lens[0], lens[1] = 0, min(M, chars.shape[1])
        out.append((np.ascontiguousarray(chars), lens))
    return out


def random_300():
    allstr, sub = synth.random_dfa(300, seed=5, total=True, n_substr_pairs=30)
    return [hra.RegexDefs(hra.AllstrRegexDef(allstr), [hra.SubstrRegexDef(sub)])]


ALL_FORMS = ("sm", "sm-pitched", "pm", "pm-in", "planes", "planes-in")
SETS = {"regex1": (lambda: defs_of_files(CFG_1), ALL_FORMS), "regex12": (lambda: defs_of_files(CFG_A), ALL_FORMS), "regex123": (lambda: defs_of_files(CFG_123), ALL_FORMS),
        "four": (lambda: defs_of_files(CFG_H4), ALL_FORMS), "eight": (lambda: defs_of_files(CFG_H4 * 2), ALL_FORMS),
        "twelve": (lambda: defs_of_files(CFG_H4 * 3), ("sm", "sm-pitched", "pm", "pm-in")), "random300": (random_300, ALL_FORMS)}


@pytest.mark.parametrize("name", list(SETS))
def test_clean_rows_every_form(name):
    """device verdict == host twin of the same rows == torch bits, all 300 strings of both batches (strings whose status word is not ok included: their rows
    are whatever the witness kernel left, and all three judge the same bytes)"""
    M = 264
    make, forms = SETS[name]
    cfg = hra.RegexVerifyConfig.configure(M, make(), device=0)
    for chars, lens in stress_batches(M):
        n_ok = None
        for form in forms:
            rows = Rows(cfg, form, chars, lens)
            assert (rows.planes is None) or len(rows.planes) == (2 if rows.D == 1 else rows.D)
            got = rows.verify()
            rec, msk = rows.host_rows()
            want = cfg.verify_rows_host(chars, lens, rec, msk)
            bad = np.nonzero(got != want)[0]
            assert not len(bad), "%s %s: string %d: %s, host twin %s" % (name, form, bad[0], hra.explain_verdict(got[bad[0]]), hra.explain_verdict(want[bad[0]]))
            assert np.array_equal((got & np.uint64(0xffffffff)).astype(np.int64), torch_bits(cfg, rows, rec, msk)), "%s %s: bits differ from the torch checker's" % (name, form)
            ok = (rows.st.cpu().numpy().view(np.uint64) & np.uint64(0xff)) == 0
            assert ((got[ok] & np.uint64(0xffffffff) & ~np.uint64(FAIL_ACCEPT)) == 0).all(), "%s %s: a string with status 0 fails a check" % (name, form)
            n_ok = int(ok.sum())
        assert n_ok > (100 if name in ("regex1", "regex12", "regex123") else 0)


@pytest.mark.parametrize("form", ["pm", "pm-in"])
def test_block_border(form):
    """65536 + 300 strings x 19 rows of sweep_def(40): the second block's string count enters the masked-row and input indices from row 8 / 16 on.  Clean: all zero
    but the accept chain; then one masked cell (row 17) and one record (row 9) of string 65536 + 5 changed on the device: exactly that string, with the host twin's word"""
    chars, lens = fc.tall_batch()
    B, M = len(lens), 19
    assert B == 65536 + 300 and chars.shape[1] == 32
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text([fc.sweep_def(fc.BIG_SWEEP_L)]), device=0)
    rows = Rows(cfg, form, chars, lens)
    assert (rows.st.cpu().numpy() & 0xff == 0).all()
    clean = rows.verify()
    assert np.array_equal(clean, rows.host_words())
    assert ((clean & np.uint64(0xffffffff) & ~np.uint64(FAIL_ACCEPT)) == 0).all() and (clean == 0).sum() > 1000
    b = 65536 + 5
    rows.set_msk(b, 17, rows.get_msk(b, 17) ^ 0x0101)
    rows.xor_rec(b, 9, 0, 1)
    got, want = rows.verify(), rows.host_words()
    assert np.array_equal(got, want)
    changed = np.nonzero(got != clean)[0]
    # (the record's row 9 lies in the string or behind it: the transition lookup of the pair (8, 9), or the padding rule)
    assert changed.tolist() == [b] and int(got[b]) & FAIL_MASK and int(got[b]) & (hra.VERIFY_TRANSITION | hra.VERIFY_PADDING), hra.explain_verdict(got[b])
    assert int(got[b]) >> 32 == min([9 if int(got[b]) & hra.VERIFY_PADDING else 8] + ([int(clean[b]) >> 32] if clean[b] else [])), hra.explain_verdict(got[b])


# ---- tamper matrix -----------------------------------------------------------------------------------------------------------------------------------
def tamper_batch(M):
    """strings regex1 + regex2 accept (clean word 0), of lengths 40 and 96, one per mutation: (chars, lens, mutations) with mutations[b] = (kind, row, def) or None"""
    texts = [b"email was meant for @" + b"y" * k + b". Also for swq." for k in (4, 60)]
    muts = [None, None]
    for text in texts:
        n = len(text)
        edge = sorted({0, 3, 4, 7, 8, 15, 16, 63, 64, 65, n - 1, n, M - 1})
        for r in edge:
            for kind in ("state", "sid", "se", "ee", "fl4", "mask"):
                for d in ((0, 1) if kind != "mask" else (0,)):
                    muts.append((text, kind, r, d))
        muts.append((text, "first", 0, 0))
        muts.append((text, "first", 0, 1))
    muts += [None, None]
    B = len(muts)
    chars = np.zeros((B, 272), np.uint8)
    lens = np.zeros(B, np.uint32)
    for b, m in enumerate(muts):
        text = texts[b % 2] if m is None else m[0]
        chars[b, :len(text)] = np.frombuffer(text, np.uint8)
        lens[b] = len(text)
    return chars, lens, [None if m is None else m[1:] for m in muts]


@pytest.mark.parametrize("form", ["sm", "pm-in", "planes"])
def test_tamper_matrix(form):
    M = 264
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=0)
    chars, lens, muts = tamper_batch(M)
    rows = Rows(cfg, form, chars, lens)
    assert (rows.verify() == 0).all()
    for b, m in enumerate(muts):
        if m is None:
            continue
        kind, r, d = m
        if kind == "mask":
            rows.set_msk(b, r, rows.get_msk(b, r) ^ 0x0101)
        else:
            rows.xor_rec(b, r, d, {"state": 1, "first": 1, "sid": 1 << 16, "se": 1 << 24, "ee": 1 << 25, "fl4": 1 << 26}[kind])
    got = rows.verify()
    rec, msk = rows.host_rows()
    want = cfg.verify_rows_host(chars, lens, rec, msk)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: string %d %s: %s, host twin %s" % (form, bad[0], muts[bad[0]], hra.explain_verdict(got[bad[0]]), hra.explain_verdict(want[bad[0]]))
    bits = (got & np.uint64(0xffffffff)).astype(np.int64)
    assert np.array_equal(bits, torch_bits(cfg, rows, rec, msk))
    seen = 0
    for b, m in enumerate(muts):
        if m is None:
            assert got[b] == 0, "string %d was not touched: %s" % (b, hra.explain_verdict(got[b]))
            continue
        kind, r, d = m
        assert got[b] != 0 and int(got[b]) >> 57 == 0, "string %d %s: not caught" % (b, m)
        assert int(got[b]) >> 32 in (r, r - 1) or kind in ("se", "ee", "sid"), "string %d %s: %s" % (b, m, hra.explain_verdict(got[b]))     # (a moved flag or tag may break a masked row before it)
        assert int(got[b]) >> 32 <= r, "string %d %s: %s" % (b, m, hra.explain_verdict(got[b]))
        seen |= int(bits[b])
    assert seen == ALL_BUT_ENABLE, "checks never seen: %s" % hra.explain_verdict(ALL_BUT_ENABLE & ~seen)


# ---- long ranges -------------------------------------------------------------------------------------------------------------------------------------
def lever_batch(M, D):
    """64 strings of the lever definitions: (chars, lens, cases) with cases[b] = (kind, first row, rows of the range) for the strings 0..3, filler behind them"""
    ko, kr = 0, D - 1
    made = [("confirmed",) + cd.sc_confirmed(M, 0, M - 3, ko, kr), ("second_start",) + cd.sc_second_start(M, 0, M - 3, ko, kr),
            ("string_end",) + cd.sc_string_end(M, 0, M - 1, ko, kr), ("reach_m",) + cd.sc_reach_m(M, 0, None, ko, kr)]
    B = 64
    chars = np.full((B, M + 16), cd.LEVERS[0][0], np.uint8)
    lens = np.full(B, M, np.uint32)
    cases = []
    for b, (kind, v, code, ranges) in enumerate(made):
        assert code == 0 and len(ranges) == 1 and ranges[0][0] == 0
        chars[b, :len(v)] = v
        lens[b] = len(v)
        cases.append((kind, ranges[0][0], ranges[0][1]))
    for b in range(B):
        chars[b, lens[b]:] = 0
    return chars, lens, cases


@pytest.mark.parametrize("D,form", [(1, "pm-in"), (3, "planes")], ids=["one-def-interleaved", "three-defs-planes"])
def test_long_ranges(D, form):
    """M = 2048.  A range of M - 2 revealed rows that an end-only event confirms (the pending rows wait 2046 rows for their verdict): clean 0; one masked cell
    blanked at row 1 / 1000 / M - 3: the masked rows, at that row.  A range that a second start, the string's end or row M takes back: clean 0 — but for the
    string that ends at M - 1, whose last state cannot be the lever DFA's accepted one without an end flag that would confirm the range: exactly the accept
    chain at row n — and with the whole range filled in as if revealed: the masked rows, at the range's first row"""
    M = 2048
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text(cd.lever_defs(D)), device=0)
    chars, lens, cases = lever_batch(M, D)
    rows = Rows(cfg, form, chars, lens)
    assert (rows.st.cpu().numpy() & 0xff == 0).all()
    clean = rows.verify()
    assert np.array_equal(clean, rows.host_words())
    for b, (kind, a, end) in enumerate(cases):
        assert clean[b] == (FAIL_ACCEPT | int(lens[b]) << 32 if kind == "string_end" else 0), (kind, hra.explain_verdict(clean[b]))
    assert (clean[4:] == 0).all()
    rec, msk = rows.host_rows()
    assert (msk[0, :M - 2] != 0).all() and not msk[1:4].any()
    f = int(cd.LEVERS[0][0])
    for row in (1, 1000, M - 3):
        keep = rows.get_msk(0, row)
        rows.set_msk(0, row, 0)
        got = rows.verify()
        assert np.array_equal(got, rows.host_words()) and got[0] == (FAIL_MASK | row << 32) and np.array_equal(got[1:], clean[1:]), hra.explain_verdict(got[0])
        rows.set_msk(0, row, keep)
    assert np.array_equal(rows.verify(), clean)
    for b in (1, 2, 3):
        kind, a, end = cases[b]
        for r in range(a, min(end, int(lens[b]))):        # as if revealed: the byte with the row's own substring id (Sum(substr_id) over the defs: the s row carries def 0's id)
            rows.set_msk(b, r, int(chars[b, r]) | int(((rec[b, r] >> 16) & 0xff).sum()) << 8)
    got = rows.verify()
    assert np.array_equal(got, rows.host_words())
    for b in (1, 2, 3):
        assert int(got[b]) & 0xffffffff == (FAIL_MASK | (int(clean[b]) & 0xffffffff)) and int(got[b]) >> 32 == cases[b][1], (cases[b], hra.explain_verdict(got[b]))
    assert got[0] == 0 and (got[4:] == 0).all()


# ---- contract ----------------------------------------------------------------------------------------------------------------------------------------
def small_rows(cfg_of=None, form="pm-in", M=64, B=70):
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=0) if cfg_of is None else cfg_of
    chars, lens = synth.ragged(B, M, seed=3)
    return Rows(cfg, form, np.ascontiguousarray(chars), lens)


def test_too_long_a_string_gives_all_ones():
    for form in ("sm", "pm-in", "planes"):
        rows = small_rows(form=form)
        clean = rows.verify()
        lens = rows.lens.copy()
        lens[33] = rows.M + 1
        got = rows.verify(lens=torch.from_numpy(lens.astype(np.int32)).to(DEV))
        assert got[33] == np.uint64(0xffffffffffffffff) and np.array_equal(np.delete(got, 33), np.delete(clean, 33))
        assert np.array_equal(got, rows.host_words(lens=lens))


def test_capture_and_replay():
    """a fresh context inside a capture: HRX_ERR_STATE and nothing written; after one eager call the launch captures, and replays with the same verdicts"""
    rows = small_rows()
    raw, v = guarded(rows.B)
    side = torch.cuda.Stream(DEV)
    dummy = torch.zeros(16, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                 # no verify call before this one
        dummy.add_(1)
        with pytest.raises(hra.HrxError) as e:
            rows.cfg.verify_rows(rows.src, rows.d_lens, rows.rec, rows.msk, layout=rows.layout, out=v, stream=side, **rows.kw)
    assert e.value.code == hra.HRX_ERR_STATE
    g.replay()
    torch.cuda.synchronize()
    assert bool((raw == POISON).all())
    want = rows.verify()                                   # the eager call: builds and uploads the tables
    assert np.array_equal(want, rows.host_words())
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side):
        rows.cfg.verify_rows(rows.src, rows.d_lens, rows.rec, rows.msk, layout=rows.layout, out=v, stream=side, **rows.kw)
    torch.cuda.synchronize()
    assert bool((raw == POISON).all())                     # captured, not run
    for _ in range(2):
        g2.replay()
        torch.cuda.synchronize()
        assert np.array_equal(v.cpu().numpy().view(np.uint64), want) and guards_intact(raw, rows.B)
        v.fill_(POISON)


def test_refused_calls_write_nothing():
    import ctypes as C
    rows = small_rows(form="planes-in")
    cfg, B, M = rows.cfg, rows.B, rows.M
    raw, v = guarded(B)
    lib, ctx = hra.lib, cfg._ctx
    arr = (C.c_void_p * 2)(*[p.data_ptr() for p in rows.planes])
    common = (rows.src.data_ptr(), rows.stride, rows.d_lens.data_ptr())
    assert lib.hrx_verify_rows_device_planes(ctx, PM_IN, *common, arr, 2, rows.msk.data_ptr(), B, M, v.data_ptr(), None) == hra.HRX_OK
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy().view(np.uint64), rows.host_words()) and guards_intact(raw, B)
    v.fill_(POISON)
    assert lib.hrx_verify_rows_device_planes(ctx, PM_IN, *common, arr, 2, rows.msk.data_ptr(), B, M, v.data_ptr() + 4, None) == hra.HRX_ERR_ARG      # misaligned verdict
    assert lib.hrx_verify_rows_device_planes(ctx, hra.LAYOUT_STRING_MAJOR, *common, arr, 2, rows.msk.data_ptr(), B, M, v.data_ptr(), None) == hra.HRX_ERR_ARG
    assert lib.hrx_verify_rows_device_planes(ctx, PM_IN, *common, arr, 1, rows.msk.data_ptr(), B, M, v.data_ptr(), None) == hra.HRX_ERR_ARG          # wrong plane count
    assert lib.hrx_verify_rows_device_planes(ctx, PM_IN, *common, arr, 3, rows.msk.data_ptr(), B, M, v.data_ptr(), None) == hra.HRX_ERR_ARG
    null = (C.c_void_p * 2)(rows.planes[0].data_ptr(), None)
    assert lib.hrx_verify_rows_device_planes(ctx, PM_IN, *common, null, 2, rows.msk.data_ptr(), B, M, v.data_ptr(), None) == hra.HRX_ERR_ARG         # NULL plane
    assert lib.hrx_verify_rows_device_planes(ctx, PM_IN, *common, None, 2, rows.msk.data_ptr(), B, M, v.data_ptr(), None) == hra.HRX_ERR_ARG
    assert lib.hrx_verify_rows_device_planes(ctx, PM_IN, *common, arr, 2, rows.msk.data_ptr(), B, (1 << 24) + 1, v.data_ptr(), None) == hra.HRX_ERR_ARG
    assert lib.hrx_verify_rows_device_planes(ctx, PM_IN, rows.src.data_ptr() + 4, *common[1:], arr, 2, rows.msk.data_ptr(), B, M, v.data_ptr(), None) == hra.HRX_ERR_ARG
    sm = small_rows(cfg_of=cfg, form="sm")
    args = (sm.src.data_ptr(), sm.stride, sm.d_lens.data_ptr(), sm.rec.data_ptr())
    assert lib.hrx_verify_rows_device(ctx, 0, *args, M - 1, sm.msk.data_ptr(), 0, B, M, v.data_ptr(), None) == hra.HRX_ERR_ARG                           # pitch < M
    assert lib.hrx_verify_rows_device(ctx, 4, *args, 0, sm.msk.data_ptr(), 0, B, M, v.data_ptr(), None) == hra.HRX_ERR_ARG
    assert lib.hrx_verify_rows_device(ctx, 0, *args, 0, None, 0, B, M, v.data_ptr(), None) == hra.HRX_ERR_ARG
    host_only = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=hra.HRX_DEVICE_NONE)
    assert lib.hrx_verify_rows_device(host_only._ctx, 0, *args, 0, sm.msk.data_ptr(), 0, B, M, v.data_ptr(), None) == hra.HRX_ERR_HIP
    assert lib.hrx_verify_rows_device_planes(host_only._ctx, PM_IN, *common, arr, 2, rows.msk.data_ptr(), B, M, v.data_ptr(), None) == hra.HRX_ERR_HIP
    torch.cuda.synchronize()
    assert bool((raw == POISON).all())
    assert lib.hrx_verify_rows_device(ctx, 0, *args, 0, sm.msk.data_ptr(), 0, B, M, v.data_ptr(), None) == hra.HRX_OK
    torch.cuda.synchronize()
    want = sm.host_words()
    assert np.array_equal(v.cpu().numpy().view(np.uint64), want) and guards_intact(raw, B)
    # a clone builds tables of its own at its first call
    got = cfg.clone().verify_rows(sm.src, sm.d_lens, sm.rec, sm.msk)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want)
