"""Field cells (hrx_fr_columns_device / _planes, fr_columns_kernel of csrc/hrx_kernel.hip) against F::from of the ORACLE's rows, bit for bit, where the kernel
can be wrong without the rest of the suite noticing (cases and reference: tests/fr_cases.py, asserted without a GPU by tests/test_fr_cases_cpu.py):

  1. state values >= 256, which the kernel computes in place instead of reading from its LDS table   test_big_states_every_form
  2. strings of the second block of 65536 of the position-major buffers (blk0, nb, bl)                test_block_border_and_launch_cut, .._two_defs, .._19_rows
  3. the 32768-string launch cut at b_begin != 0, alone and together with the block border           test_block_border_and_launch_cut
  4. 4 .. 8 defs (interleaved records and record planes), 12 and 13 defs (interleaved)               test_def_counts
  5. row counts around a store (32), a wave (128), a block (512), partial quads and octets           test_row_count_edges
  6. a guard before and behind the cells in every test; calls the library refuses write nothing      test_refused_calls_write_nothing

Every test runs the witness kernels first (their status words must equal the oracle's), then fr_columns of their rows into guarded cells, Montgomery and
canonical, and compares every string of the request.  Only test_out_of_contract_strings_do_no_harm holds strings whose status is not 0, and names them."""
import re

import numpy as np
import pytest

import fr_cases as fc
from oracle_lib import DFA_DIR, OracleDefs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hra():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    import halo2_regex_amd as m
    return m


def _defs_of_files(hra, names):
    return [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(DFA_DIR + "/" + a), [hra.SubstrRegexDef.read_from_text(DFA_DIR + "/" + s) for s in subs]) for a, subs in names]


def _defs_of_text(hra, defs_t):
    return [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs in defs_t]


class Batch:
    """one case: the config on the device, the batch in both input layouts, the oracle's status words and expected columns"""

    def __init__(self, hra, o, defs, chars, lens, M, threads=1):
        import torch
        self.hra, self.torch, self.dev = hra, torch, torch.device("cuda", 0)
        self.M, self.D, self.B, self.stride = M, o.D, len(lens), chars.shape[1]
        self.chars, self.lens = chars, lens
        self.cfg = hra.RegexVerifyConfig.configure(M, defs, device=0)
        self.orec, self.omsk, self.ost = o.witness_batch(chars, lens, M, threads=threads)
        self.ok = np.nonzero((self.ost & np.uint64(0xff)) == 0)[0]
        self.cols = fc.expected_columns(self.orec, self.omsk, chars, lens, M, self.D)
        self.d_chars = torch.from_numpy(chars).to(self.dev)
        self.d_lens = torch.from_numpy(lens.astype(np.int32)).to(self.dev)
        self.d_chars_pm = hra.chars_to_position_major(self.d_chars)
        self._want = {}

    def want(self, canonical, b_begin=0, b_count=None):
        b_count = self.B - b_begin if b_count is None else b_count
        key = (canonical, b_begin, b_count)
        if key not in self._want:
            if len(self._want) > 8:
                self._want.clear()
            self._want[key] = fc.cells_of(self.cols[:, b_begin:b_begin + b_count], canonical)
        return self._want[key]

    def witness(self, form, check_rows=True):
        """Runs the witness kernels for `form` -> (src, out, kw) as fr_columns takes them.  Forms: sm / sm-pitched (string-major, tight / recommended pitches),
        pm / pm-in (position-major interleaved records from string-major / position-major input), planes / planes-in (record planes, or at one def the two
        row stripes, from the two input layouts).  The status words, and with check_rows the rows, must be the oracle's."""
        hra, torch, cfg, B, M, D = self.hra, self.torch, self.cfg, self.B, self.M, self.D
        pm_in = dict(chars_pm_stride=self.stride)
        if form in ("sm", "sm-pitched"):
            out = cfg.witness_batch(self.d_chars, self.d_lens, out=cfg.alloc_outputs(B, self.dev, pitched=form == "sm-pitched"))
            src, kw, rows = self.d_chars, dict(position_major=False), (out[0], out[1])
            assert form == "sm" or out[0].stride(0) // D == hra.recommended_pitches(M)[0]
        elif form in ("pm", "pm-in"):
            src, kw = (self.d_chars_pm, pm_in) if form == "pm-in" else (self.d_chars, {})
            out = cfg.witness_batch_position_major(src, self.d_lens, **kw)
            rows = hra.position_major_to_string_major(out[0], out[1], B, M, D) if check_rows else None
            kw = dict(position_major=True, **kw)
        else:
            assert form in ("planes", "planes-in")
            src, kw = (self.d_chars_pm, pm_in) if form == "planes-in" else (self.d_chars, {})
            out = cfg.witness_batch_planes(src, self.d_lens, out=cfg.alloc_output_planes(B, self.dev, stripes=2 if D == 1 else None), **kw)
            assert len(out[0]) == (2 if D == 1 else D)
            rows = hra.planes_to_string_major(out[0], out[1], B, M, D) if check_rows else None
            kw = dict(position_major=True, **kw)
        torch.cuda.synchronize()
        st = out[2].cpu().numpy().view(np.uint64)
        assert np.array_equal(st, self.ost), "%s: status words differ from the oracle's, first at string %d" % (form, int(np.nonzero(st != self.ost)[0][0]))
        if check_rows:
            rec, msk = rows[0].cpu().numpy().view(np.uint32), rows[1].cpu().numpy().view(np.uint16)
            assert np.array_equal(rec[self.ok], self.orec[self.ok]) and np.array_equal(msk[self.ok], self.omsk[self.ok]), form + ": the witness rows differ from the oracle's"
        return src, out, kw

    def check(self, src, out, kw, tag, b_begin=0, b_count=None, keep=None, on_device=False):
        """fr_columns of strings [b_begin, b_begin + b_count) into guarded cells, Montgomery and canonical, against F::from of the oracle's columns;
        keep: the strings of the request that are compared (default: every one)"""
        torch = self.torch
        b_count = self.B - b_begin if b_count is None else b_count
        for canonical in (False, True):
            what = "%s [%d, %d) %s" % (tag, b_begin, b_begin + b_count, "canonical" if canonical else "Montgomery")
            cells, raw = fc.guarded_cells(torch, self.dev, 4 + 4 * self.D, b_count, self.M)
            got = self.cfg.fr_columns(src, self.d_lens, out, b_begin=b_begin, b_count=b_count, canonical=canonical, cells=cells, **kw)
            torch.cuda.synchronize()
            assert got.data_ptr() == cells.data_ptr() and got.shape == (4 + 4 * self.D, b_count, self.M, 4)
            fc.guards_intact(raw, cells, what)
            want = self.want(canonical, b_begin, b_count)
            if on_device:
                w = torch.from_numpy(want.view(np.int64)).to(self.dev)
                if not torch.equal(cells, w):
                    c, b, r, k = (int(x) for x in (cells != w).nonzero()[0])
                    raise AssertionError("%s: column %d string %d row %d limb %d: got %#x want %#x" % (what, c, b_begin + b, r, k, int(cells[c, b, r, k]) & (2 ** 64 - 1), int(want[c, b, r, k])))
                continue
            got = got.cpu().numpy().view(np.uint64)
            if keep is not None:
                got, want = got[:, keep], want[:, keep]
            err = fc.first_difference(got, want)
            assert err is None, "%s: %s" % (what, err)


# ---- 1. big states ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweeps(hra, oracle):
    made = {}

    def get(D):
        if D not in made:
            defs_t = fc.sweep_defs(D)
            chars, lens = fc.sweep_batch(fc.SWEEP_L if D == 1 else fc.SWEEP_L2)
            made[D] = Batch(hra, OracleDefs(oracle, defs_t), _defs_of_text(hra, defs_t), chars, lens, 72)
        return made[D]
    return get


@pytest.mark.parametrize("D,form", [(1, "sm"), (1, "sm-pitched"), (1, "pm"), (1, "pm-in"), (1, "planes-in"), (2, "pm-in"), (2, "planes")],
                         ids=["D1-string-major", "D1-string-major-pitched", "D1-position-major", "D1-position-major-input", "D1-row-stripes", "D2-interleaved", "D2-record-planes"])
def test_big_states_every_form(hra, sweeps, D, form):
    """The sweep batch: every state value 0 .. 2046 (D = 1) / 0 .. 1021 (D = 2), 1791 / 766 of them >= 256, out of tables of 2048 / 2046 rows that only the
    global-table kernels take; the whole batch and the sub-range [7, 28)."""
    bt = sweeps(D)
    assert len(bt.ok) == bt.B == 40 and bt.cols.max() == (fc.SWEEP_L if D == 1 else fc.SWEEP_L2) + 1
    layout = {"sm": 0, "sm-pitched": 0, "pm": 1, "pm-in": 3, "planes": 1 | hra.LAYOUT_RECORD_PLANES, "planes-in": 3 | hra.LAYOUT_RECORD_PLANES}[form]
    d = bt.cfg.describe_launch(bt.B, layout=layout)
    assert re.match(r"hrx::witness_kernel<%d, (true|false), true>" % D if layout == 0 else r"hrx::witness_pm_kernel<%d, true," % D, d), d      # GLOBAL = true
    src, out, kw = bt.witness(form)
    bt.check(src, out, kw, "D=%d %s" % (D, form))
    bt.check(src, out, kw, "D=%d %s" % (D, form), b_begin=7, b_count=21)


# ---- 4. def counts ---------------------------------------------------------------------------------------------------------------------------------
def _defcount_names(name):
    import test_parity_gpu as tp
    return {"D4": tp.CFG_D4, "D5": tp.CFG_D5, "D6": tp.CFG_D6, "D7": tp.CFG_D7, "D8": tp.CFG_D8, "D13": tp.CFG_D13,
            "D12": tp.CFG_123 + tp.HDR + tp.NOSUB(tp.CFG_123 + tp.HDR)}[name]      # (D12 = D13 without the partial example DFA: every string has status 0)


@pytest.mark.parametrize("name,forms", [("D4", ("pm-in", "planes")), ("D5", ("pm", "planes-in")), ("D6", ("pm-in", "planes")), ("D7", ("pm", "planes-in")),
                                        ("D8", ("pm-in", "planes")), ("D13", ("pm", "pm-in")), ("D12", ("pm", "pm-in"))], ids=["D4", "D5", "D6", "D7", "D8", "D13", "D12"])
def test_def_counts(hra, oracle, name, forms):
    """The column arithmetic 2 + 4 d .. 3 + 4 D beyond three defs: interleaved records and record planes at 4 .. 8 defs, interleaved records (multi-pass
    configs) at 12 and 13; 70 strings x 72 rows, the oracle's status-0 strings (at least the share tests/test_parity_gpu.py asks of these configs, and 2/3).
    At D7 and D13 the status-0 strings are prefixes of one literal and header lines that reveal nothing, so columns 2 + 4 D and 3 + 4 D are almost all zero there:
    D12 (D13 without the partial example DFA, every string status 0, more than 400 nonzero masked rows) is the case that checks those two columns past 8 defs."""
    names = _defcount_names(name)
    chars, lens = fc.defcount_batch(names)
    bt = Batch(hra, OracleDefs.from_files(oracle, names), _defs_of_files(hra, names), chars, lens, 72)
    assert bt.D == int(name[1:]) and len(bt.ok) >= 70 * max(2 / 3, 0.5 if name in ("D4", "D5", "D6") else 0)
    for form in forms:
        src, out, kw = bt.witness(form)
        bt.check(src, out, kw, "%s %s" % (name, form), keep=bt.ok)


# ---- 5. row-count edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", fc.EDGE_MS)
def test_row_count_edges(hra, oracle, M):
    """regex1 + regex2, five strings of lengths {0, 1, M - 1, M, M // 2} with planted matches, every form that exists at two defs"""
    chars, lens, stride = fc.edge_batch(M)
    bt = Batch(hra, OracleDefs.from_files(oracle, fc.CFG_A), _defs_of_files(hra, fc.CFG_A), chars, lens, M)
    assert len(bt.ok) == 5 and stride > M and stride % 16 == 0
    for form in ("sm", "sm-pitched", "pm", "pm-in", "planes"):
        src, out, kw = bt.witness(form)
        bt.check(src, out, kw, "M=%d %s" % (M, form))


# ---- 2., 3. block border and launch cut ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bigs(hra, oracle):
    made = {}

    def get(case):
        if case not in made:
            made.clear()      # (one at a time: each holds some 100 MB)
            if case in ("sweep40", "sweep40-tall"):
                defs_t = [fc.sweep_def(fc.BIG_SWEEP_L)]
                o, defs, alphabet = OracleDefs(oracle, defs_t), _defs_of_text(hra, defs_t), fc.BIG_SWEEP_BYTES
            else:
                names = fc.CFG_1 if case == "regex1" else fc.CFG_A
                o, defs, alphabet = OracleDefs.from_files(oracle, names), _defs_of_files(hra, names), None
            chars, lens = fc.tall_batch() if case == "sweep40-tall" else fc.big_batch(alphabet)
            made[case] = Batch(hra, o, defs, chars, lens, fc.TALL_M if case == "sweep40-tall" else fc.BIG_M, threads=8)
        return made[case]
    return get


@pytest.mark.parametrize("form", ["pm", "pm-in", "planes-in", "sm"], ids=["position-major", "position-major-input", "row-stripes", "string-major"])
@pytest.mark.parametrize("case", ["regex1", "sweep40"])
def test_block_border_and_launch_cut(hra, bigs, case, form):
    """65536 + 300 strings x 8 rows, one def: requests on both sides of the position-major buffers' block border (the second block holds nb = 300 strings),
    one string each side of it, the batch's last string, [30000, 65800) across the launch cut at 30000 + 32768 and the border (compared on the device), and no
    string at all.  String-major: the launch cut alone.  regex1 reveals nothing within 8 rows (its public part begins after 21 literal bytes), so the same
    requests run on sweep_def(40) too, whose masked rows are nonzero on both sides of the border."""
    bt = bigs(case)
    assert bt.B == 65536 + 300 and len(bt.ok) == bt.B and bt.stride == 16 and bt.D == 1
    assert bool(bt.cols[6].any()) == (case == "sweep40")
    src, out, kw = bt.witness(form, check_rows=False)
    tag = "%s %s" % (case, form)
    if form == "sm":
        bt.check(src, out, kw, tag, 30000, 35800, on_device=True)
        return
    for b_begin, b_count in fc.BIG_RANGES:
        bt.check(src, out, kw, tag, b_begin, b_count, on_device=b_count > 1000)


@pytest.mark.parametrize("form", ["pm", "pm-in", "planes-in"], ids=["position-major", "position-major-input", "row-stripes"])
def test_block_border_19_rows(hra, bigs, form):
    """At 8 rows the string count nb = 300 of the second block is multiplied by zero in the masked-row index ((r >> 3) * nb) and in the position-major chars
    index ((r >> 4) * nb).  65536 + 300 strings x 19 rows of sweep_def(40) reach masked octets 1 and 2 and chars group 1 there, nonzero on both sides of the
    border (tests/test_fr_cases_cpu.py shows that nb - 1 in either index would read other values in each of the three short requests)."""
    bt = bigs("sweep40-tall")
    assert bt.B == 65536 + 300 and len(bt.ok) == bt.B and bt.M == 19 and bt.stride == 32 and bt.D == 1
    assert bt.cols[6, 65536:, 8:].any() and bt.cols[1, 65536:, 16].any()
    src, out, kw = bt.witness(form, check_rows=False)
    for b_begin, b_count in fc.BIG_SHORT:
        bt.check(src, out, kw, "19 rows " + form, b_begin, b_count)


@pytest.mark.parametrize("form", ["pm-in", "planes"], ids=["interleaved", "record-planes"])
def test_block_border_two_defs(hra, bigs, form):
    bt = bigs("regex12")
    assert bt.D == 2 and len(bt.ok) == bt.B
    src, out, kw = bt.witness(form, check_rows=False)
    for b_begin, b_count in fc.BIG_SHORT:
        bt.check(src, out, kw, "D=2 " + form, b_begin, b_count)


# ---- out-of-contract strings, refused calls --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bad(hra, oracle):
    chars, lens = fc.bad_batch()
    return Batch(hra, OracleDefs.from_files(oracle, fc.CFG_A), _defs_of_files(hra, fc.CFG_A), chars, lens, 72)


@pytest.mark.parametrize("form", ["sm", "pm-in", "planes"])
def test_out_of_contract_strings_do_no_harm(hra, bad, form):
    """Strings 3 and 40 have lens = M + 1, string 9 a byte without a transition: the call returns, the guards are intact, every other string equals the reference"""
    bt = bad
    keep = np.array([b for b in range(70) if b not in fc.BAD_STRINGS])
    assert np.array_equal(bt.ok, keep) and len(keep) == 67
    src, out, kw = bt.witness(form)
    bt.check(src, out, kw, "out of contract " + form, keep=keep)


def test_refused_calls_write_nothing(hra, bad):
    import torch
    bt, cfg = bad, bad.cfg
    B, M, D = bt.B, bt.M, bt.D
    out_sm = bt.witness("sm")[1]
    _, out_pm, kw_pm = bt.witness("pm")
    _, out_pl, _ = bt.witness("planes")
    refused = []

    def refuse(what, match, call, b_count, offset=0):
        cells, raw = fc.guarded_cells(torch, bt.dev, 4 + 4 * D, b_count, M, offset=offset)
        with pytest.raises(hra.HrxError, match=match):
            call(cells)
        torch.cuda.synchronize()
        assert fc.untouched(raw), what + ": a refused call wrote"
        refused.append(what)

    refuse("misaligned cells", "16-byte aligned", lambda c: cfg.fr_columns(bt.d_chars, bt.d_lens, out_sm, cells=c), B, offset=8)
    refuse("range behind the batch", "string range outside the batch", lambda c: cfg.fr_columns(bt.d_chars, bt.d_lens, out_sm, b_begin=60, b_count=11, cells=c), 11)
    refuse("range behind the batch, position-major", "string range outside the batch", lambda c: cfg.fr_columns(bt.d_chars, bt.d_lens, out_pm, b_begin=B, b_count=1, cells=c, **kw_pm), 1)
    refuse("planes, string-major layout", "position-major layout", lambda c: cfg.fr_columns(bt.d_chars, bt.d_lens, out_pl, position_major=False, cells=c), B)
    three = (list(out_pl[0]) + [out_pl[0][0]], out_pl[1], out_pl[2])
    refuse("three planes for two defs", "record planes", lambda c: cfg.fr_columns(bt.d_chars, bt.d_lens, three, position_major=True, cells=c), B)
    one = ([out_pl[0][0]], out_pl[1], out_pl[2])
    refuse("one plane for two defs", "record planes", lambda c: cfg.fr_columns(bt.d_chars, bt.d_lens, one, position_major=True, cells=c), B)

    def layout_2(c):      # position-major input alone is no layout of this call: the Python mirror cannot say it
        s = torch.cuda.current_stream(bt.dev)
        hra._check(hra.lib.hrx_fr_columns_device(cfg._need_ctx(), hra.LAYOUT_INPUT_POSITION_MAJOR, bt.d_chars_pm.data_ptr(), bt.stride, bt.d_lens.data_ptr(), out_pm[0].data_ptr(), 0,
                                                 out_pm[1].data_ptr(), 0, B, M, 0, B, c.data_ptr(), 0, s.cuda_stream))
    refuse("layout 2", "unknown layout", layout_2, B)
    # the Python mirror refuses a cells tensor of another size or type before the library sees it
    refuse("cells of another size", "cells", lambda c: cfg.fr_columns(bt.d_chars, bt.d_lens, out_sm, b_count=B - 1, cells=c), B)
    assert len(refused) == 8
