"""HRX_OPT_MATCH_FUSED_WIDE (include/hrx.h) on host-only contexts: the option itself (default 0, round trip, clone, bad value), the describe
texts — unchanged with the option at 0, the fused-wide kernel named with it at 1 for every input form the plan allows and "via rows" for every one it does
not — host results unaffected, and the lane core of csrc/hrx_match_wide.h as a stand-alone program under the sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fuzz_defs as fd
import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import DFA_DIR
from test_match_cpu import CFG_1, CFG_23, CFG_H3, CFG_H4, _cfg, _defs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = 6
SEL, RAG, PM = 16, 8, 2
FUZZ_SEEDS = list(range(6))      # of fuzz_defs.make_case, per def count: tests/test_match_wide_gpu.py walks these on the device
LAYOUTS = {0: ("hrx::PaddedSrc", "false"), RAG: ("hrx::RaggedSrc", "false"), SEL | 0: ("hrx::PaddedSrc", "true"), SEL | RAG: ("hrx::RaggedSrc", "true")}


def wide(names, M, value=1, flags=None):
    before = os.environ.get("HRX_DEBUG_FLAGS")
    if flags is not None:
        os.environ["HRX_DEBUG_FLAGS"] = str(flags)
    try:
        cfg = _cfg(names, M)
    finally:
        if flags is not None:
            os.environ.pop("HRX_DEBUG_FLAGS")
            if before is not None:
                os.environ["HRX_DEBUG_FLAGS"] = before
    cfg.set_option(OPT, value)
    return cfg


def fuzz_cfg(case, value=1, device=hra.HRX_DEVICE_NONE):
    defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
    cfg = hra.RegexVerifyConfig.configure(case.M, defs, device=device)
    cfg.set_option(OPT, value)
    return cfg


def test_the_option_defaults_to_zero_round_trips_and_travels_with_a_clone():
    assert hra.OPT_MATCH_FUSED_WIDE == OPT
    cfg = _cfg(CFG_H4, 1024)
    assert cfg.get_option(OPT) == 0
    cfg.set_option(OPT, 1)
    assert cfg.get_option(OPT) == 1
    c = cfg.clone()
    assert c.get_option(OPT) == 1 and c.describe_match(300, layout=RAG).startswith("hrx::match_wide_kernel<4, ")
    cfg.set_option(OPT, 0)
    assert cfg.get_option(OPT) == 0 and c.get_option(OPT) == 1 and cfg.clone().get_option(OPT) == 0
    for bad in (2, -1, 7):
        with pytest.raises(hra.HrxError):
            cfg.set_option(OPT, bad)
    assert cfg.get_option(OPT) == 0
    # the three places that name the constant agree
    assert "HRX_OPT_MATCH_FUSED_WIDE = 6" in open(os.path.join(ROOT, "include", "hrx.h")).read()
    assert "pub const HRX_OPT_MATCH_FUSED_WIDE: c_int = 6;" in open(os.path.join(ROOT, "bindings", "rust", "hrx.rs")).read()


def test_option_zero_leaves_the_four_def_texts_as_they_are():
    """the shapes tests/test_select_cpu.py pins, through a context that set the option and took it back"""
    cfg = wide(CFG_H4, 1024, 1)
    cfg.set_option(OPT, 0)
    assert cfg.describe_match(65536) == ("via rows, 2 slice(s) of 43690 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + "
                                         "hrx::spans_from_masked_pm_kernel")
    assert cfg.describe_match(300, layout=RAG) == ("via rows, 1 slice(s) of 300 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 "
                                                   "ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel")
    assert cfg.describe_match(65536, layout=SEL) == ("via rows, 2 slice(s) of 41382 strings: hrx::selected_slice_kernel<hrx::PaddedSrc> + "
                                                     "hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_selected_kernel")
    assert cfg.describe_match(300, layout=SEL | RAG) == ("via rows, 1 slice(s) of 300 strings: hrx::selected_slice_kernel<hrx::RaggedSrc> + "
                                                         "hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_selected_kernel")
    big = wide(CFG_H4, 32768, 0)
    assert big.describe_match(4500, layout=PM) == ("via rows, 4 slice(s) of 1365 strings: hrx::pm_input_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 "
                                                   "ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel")
    # the context-free describe has no option
    import ctypes as C
    buf = C.create_string_buffer(4096)
    assert hra.lib.hrx_describe_match(wide(CFG_H4, 1024)._defs.h, RAG, 300, 1024, 256, buf, 4096) == hra.HRX_OK and buf.value.decode().startswith("via rows, 1 slice(s) of 300 ")


def test_option_one_names_the_fused_wide_kernel():
    cfg = wide(CFG_H4, 1024)
    lds = None
    for B in (300, 65536, 4 * 65536):
        for layout, (src, sel) in LAYOUTS.items():
            text = cfg.describe_match(B, layout=layout)
            head, tail = text.split(" grid=")
            assert head.startswith("hrx::match_wide_kernel<4, ") and head.endswith(", %s, %s>" % (src, sel)), text
            assert int(head.split(", ")[1]) == (1 if B > 65536 else 4)       # four defs: one by one past a wave per SIMD (256 CUs x 256 lanes), else four side by side
            assert tail.startswith("persistent threads=256 lds="), text
            lds = lds or int(tail.split("lds=")[1])
            assert int(tail.split("lds=")[1]) == lds and lds % 16 == 0 and 0 < lds <= 160 * 1024
    for D in (5, 8):
        names = (CFG_H4 * 2)[:D]
        for B in (4096, 4 * 65536):
            assert wide(names, 1024).describe_match(B, layout=RAG).startswith("hrx::match_wide_kernel<%d, 4, " % D)


def test_option_one_stays_via_rows_where_the_plan_says_so():
    """position-major input, more than eight defs, HRX_DEBUG_FLAGS bit 32, a def of more than 32 byte classes.  A chunked shape: the witness planner chunks no
    shape of four or more defs (its launches for them are the def-parallel kernel or passes, neither of which is ever chunked: hrx_plan.cpp), which the
    sweep below confirms through describe_launch — so there is no such case to pin"""
    cfg = wide(CFG_H4, 1024)
    for B in (300, 65536):
        assert cfg.describe_match(B, layout=PM) == wide(CFG_H4, 1024, 0).describe_match(B, layout=PM) and cfg.describe_match(B, layout=PM).startswith("via rows, ")
    assert wide(CFG_H4 * 3, 1024).describe_match(4096, layout=RAG).startswith("via rows")
    assert wide(CFG_H4, 1024, flags=1 << 32).describe_match(4096, layout=RAG).startswith("via rows")
    assert wide(CFG_H4, 1024, flags=1 << 32).describe_match(4096, layout=SEL).startswith("via rows")
    # a def whose 40 bytes each lead somewhere else from state 0: more than 32 classes, no class-wide image
    fan = "0\n40\n40\n" + "".join("0 %d %d\n" % (c + 1, 48 + c) for c in range(40))
    many = [hra.RegexDefs(hra.AllstrRegexDef(fan), [])] + _defs(CFG_H3)
    c4 = hra.RegexVerifyConfig.configure(1024, many, device=hra.HRX_DEVICE_NONE)
    c4.set_option(OPT, 1)
    assert c4.describe_match(4096, layout=RAG).startswith("via rows") and "witness_pmd_kernel" not in c4.describe_match(4096, layout=RAG)
    for M in (1024, 4096, 32768, 1 << 20):
        big = wide(CFG_H4, M)
        for B in (1, 64, 300, 4500, 8192, 65536):
            assert "chunked" not in big.describe_launch(B, layout=hra.LAYOUT_POSITION_MAJOR), (M, B)
            assert big.describe_match(B, layout=RAG).startswith("hrx::match_wide_kernel<4, "), (M, B)


def test_up_to_three_defs_are_untouched():
    for names in (CFG_1, CFG_23, CFG_H3):
        for M, B in ((1024, 65536), (1024, 300), (32768, 4500)):
            off, on = wide(names, M, 0), wide(names, M, 1)
            for layout in (0, PM, RAG, SEL, SEL | RAG):
                assert on.describe_match(B, layout=layout) == off.describe_match(B, layout=layout)
                assert "match_wide_kernel" not in on.describe_match(B, layout=layout)


def test_host_results_do_not_depend_on_the_option():
    M = 208
    chars, lens = synth.headers_planted(300, M - 1, seed=3, stride=M)
    lens = lens.astype(np.uint32)
    lens[::13] = M + 1
    off, on = wide(CFG_H4, M, 0), wide(CFG_H4, M, 1)
    a, b = off.match_batch_host(chars, lens, max_spans=8), on.match_batch_host(chars, lens, max_spans=8)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and int(a[1].sum()) > 100


@pytest.mark.parametrize("D", [4, 5, 6, 7, 8])
def test_the_gpu_tests_fuzz_cases_are_all_fused(D):
    """tests/test_match_wide_gpu.py relies on this: every def of these fuzz cases has at most 32 byte classes, so none of them falls back"""
    for seed in FUZZ_SEEDS:
        case = fd.make_case(seed, fd.Shape(D, D, "small", "any"))
        cfg = fuzz_cfg(case)
        for layout in LAYOUTS:
            assert cfg.describe_match(case.B, layout=layout).startswith("hrx::match_wide_kernel<%d, " % D), (D, seed)


def test_lane_core_as_a_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_match_wide_host.cpp: MatchLaneWide / WideAcc / wide_status (csrc/hrx_match_wide.h) over the class-wide tables of the four header
    defs, of six and of eight (the set twice over: overlaps), every sweep width, against hrx_match_batch_host's native walk; image and outputs are heap blocks
    of exactly their sizes"""
    M, B = 200, 330
    chars, lens = synth.headers_planted(B, M, seed=3, stride=208)
    edge = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, M - 1, M, M + 1]
    lens = lens.astype(np.uint32)
    lens[:len(edge) * 5] = np.array(edge * 5, np.uint32)
    chars[np.arange(208)[None, :] >= lens.astype(np.int64)[:, None]] = 0
    chars[7, 30] = 0xff          # bytes no def knows: the first undefined transition
    chars[40, 0] = 0x01
    chars[41, 199] = 0x80
    path = str(tmp_path / "batch.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4I", B, 208, M, len(CFG_H4)))
        for a, subs in CFG_H4:
            f.write(struct.pack("<I", len(subs)))
            for name in [a] + subs:
                text = open(os.path.join(DFA_DIR, name), "rb").read()
                f.write(struct.pack("<I", len(text)) + text)
        f.write(lens.tobytes() + np.ascontiguousarray(chars).tobytes())
    exe = str(tmp_path / "hrx_test_match_wide_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_match_wide_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0 and "match wide host: ok" in out.stdout, out.stdout + out.stderr
