"""CHUNKED VERIFY on the host (include/hrx.h hrx_verify_rows_chunked_host, hrx_verify_chunked_workspace_bytes, hrx_ctx_verify_chunk_rows; the chunk walk and
fold of csrc/hrx_verify.hpp): the word of every string must be the unchunked host word (hrx_verify_rows_host — the definition), bit for bit, whatever the
chunk size; the yardstick is never the chunked code.

  stress batches        the reveal-stress and ragged batches of tests/test_verify_cpu.py on its four def sets, every string whatever its status word says
  catalogue             every def set of tests/verify_cases.py at M = 139, clean and with the catalogue applied: its edge rows sit at 31 / 32 / 33 and 63 / 64 / 65
  rows 96 and 128       one-cell changes at rows 95 .. 97 and 127 .. 129 (the borders of 32-row chunks the catalogue does not reach), held to the unchunked word
  contract              the workspace size, the context's pick, the refusals of the host entry
  stand-alone program   tests/host_cpp/test_verify_chunk_host.cpp under the address and undefined-behaviour sanitizers

No device."""
import os
import subprocess

import numpy as np
import pytest

import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import ROOT
from test_mock_prover import CFG_1, CFG_3, CFG_A, CFG_123, _cfg
from test_verify_cases_cpu import expected
import verify_cases as vc

CHUNKS = (32, 64, 128, 0)
FAR_ROWS = (95, 96, 97, 127, 128, 129)
# (kind, keep, flip) of verify_cases.OPS that change a record or a masked cell
FAR_KINDS = ("state", "sid", "se", "ee", "fl2", "mask", "mask_sid")


def same_words(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: string %d: %s, unchunked %s (%d strings differ)" % (what, bad[0], hra.explain_verdict(got[bad[0]]), hra.explain_verdict(want[bad[0]]), len(bad))


def far_row_batch(name):
    """the n = 139 base string of a verify_cases set, one copy per (kind, row of FAR_ROWS, def) and two untouched: (chars, lens, [(string, kind, row, def)])"""
    cat = vc.Catalogue(name)
    v, _ = vc.base_string(name, cat.M, cat.M)
    muts = [(kind, r, d) for r in FAR_ROWS for kind in FAR_KINDS for d in (range(cat.D) if vc.OPS[kind][0] == "rec" else (0,))]
    B = len(muts) + 2
    chars = np.zeros((B, cat.stride), np.uint8)
    chars[:, :len(v)] = v
    return cat, chars, np.full(B, cat.M, np.uint32), [(b + 1,) + m for b, m in enumerate(muts)]


def apply_far(muts, rec, msk):
    rec, msk = rec.copy(), msk.copy()
    for b, kind, r, d in muts:
        buf, keep, flip = vc.OPS[kind]
        if buf == "rec":
            rec[b, r, d] = (int(rec[b, r, d]) & keep) ^ flip
        else:
            msk[b, r] = (int(msk[b, r]) & keep) ^ flip
    return rec, msk


def test_exports_and_keywords_exist():
    """(what fails first where the feature is missing)"""
    for s in ("hrx_verify_chunked_workspace_bytes", "hrx_ctx_verify_chunk_rows", "hrx_verify_rows_chunked_device", "hrx_verify_rows_chunked_device_planes",
              "hrx_verify_rows_chunked_host"):
        assert s in hra.ABI_SYMBOLS
    import inspect
    assert "chunk_rows" in inspect.signature(hra.RegexVerifyConfig.verify_rows_host).parameters
    assert {"chunk_rows", "workspace"} <= set(inspect.signature(hra.RegexVerifyConfig.verify_rows).parameters)


@pytest.mark.parametrize("names", [CFG_1, CFG_3, CFG_A, CFG_123], ids=["r1", "r3", "r1r2", "r1r2r3"])
def test_stress_batches_word_for_word(names):
    M = 264
    cfg = _cfg(names, M)
    for chars, lens in (synth.reveal_stress(300, 260, seed=5), synth.ragged(300, M, seed=7)):
        lens = lens.copy()
        lens[0], lens[1] = 0, min(M, chars.shape[1])
        rec, msk, st = cfg.witness_batch_host(chars, lens)
        want = cfg.verify_rows_host(chars, lens, rec, msk)
        assert (want != 0).sum() > 10
        for C in CHUNKS:
            same_words(cfg.verify_rows_host(chars, lens, rec, msk, chunk_rows=C), want, "chunk_rows %d" % C)
        # a pitched view and the position-major image of the same rows
        rp, mk = np.zeros((300, M + 40, len(names)), np.uint32), np.zeros((300, M + 24), np.uint16)
        rp[:, :M], mk[:, :M] = rec, msk
        same_words(cfg.verify_rows_host(chars, lens, rp[:, :M], mk[:, :M], chunk_rows=64), want, "pitched")
        D, q4, q8 = len(names), (M + 3) // 4, (M + 7) // 8
        r4, m8 = np.zeros((300, q4 * 4, D), np.uint32), np.zeros((300, q8 * 8), np.uint16)
        r4[:, :M], m8[:, :M] = rec, msk
        rec_pm = np.ascontiguousarray(r4.reshape(300, q4, 4, D).transpose(1, 3, 0, 2)).reshape(-1)
        msk_pm = np.ascontiguousarray(m8.reshape(300, q8, 8).transpose(1, 0, 2)).reshape(-1)
        same_words(cfg.verify_rows_host(chars, lens, rec_pm, msk_pm, layout=hra.LAYOUT_POSITION_MAJOR, chunk_rows=32), want, "position-major")


@pytest.mark.parametrize("name", list(vc.SETS))
def test_catalogue_word_for_word(name):
    """M = 139: five chunks of 32 rows (the last of 11), three of 64, two of 128; the catalogue's edge rows lie on both sides of rows 32 and 64"""
    e = expected(name)
    cat = e.cat
    cfg = hra.RegexVerifyConfig.configure(cat.M, [hra.RegexDefs(hra.AllstrRegexDef(t[0]), [hra.SubstrRegexDef(s) for s in t[1]]) for t in cat.defs_t],
                                          device=hra.HRX_DEVICE_NONE)
    assert (e.want != e.clean).sum() > 100
    for C in CHUNKS:
        same_words(cfg.verify_rows_host(cat.chars, cat.lens, e.rec, e.msk, chunk_rows=C), e.clean, "%s clean chunk_rows %d" % (name, C))
        same_words(cfg.verify_rows_host(e.chars_mut, cat.lens, e.rec_mut, e.msk_mut, chunk_rows=C), e.want, "%s catalogue chunk_rows %d" % (name, C))


@pytest.mark.parametrize("name", ["one", "three", "five", "eight"])
def test_cells_at_rows_96_and_128(name):
    cat, chars, lens, muts = far_row_batch(name)
    cfg = hra.RegexVerifyConfig.configure(cat.M, [hra.RegexDefs(hra.AllstrRegexDef(t[0]), [hra.SubstrRegexDef(s) for s in t[1]]) for t in cat.defs_t],
                                          device=hra.HRX_DEVICE_NONE)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    assert (st & np.uint64(0xff) == 0).all()
    rec2, msk2 = apply_far(muts, rec, msk)
    assert (rec2 != rec).sum() + (msk2 != msk).sum() == len(muts)
    want = cfg.verify_rows_host(chars, lens, rec2, msk2)
    assert want[0] == 0 and want[-1] == 0 and (want[1:-1] != 0).all()
    for C in CHUNKS:
        same_words(cfg.verify_rows_host(chars, lens, rec2, msk2, chunk_rows=C), want, "%s chunk_rows %d" % (name, C))


def test_workspace_bytes_and_the_contexts_pick():
    ws = hra.verify_chunked_workspace_bytes
    assert ws(300, 264, 32) == 32 * 9 * 300 and ws(300, 264, 64) == 32 * 5 * 300 and ws(300, 264, 256) == 32 * 2 * 300
    assert ws(300, 264, 288) == 32 * 300 and ws(300, 264, 1 << 20) == 32 * 300 and ws(1, 32, 32) == 32 and ws(0, 64, 32) == 0
    assert ws(300, 264, 0) == 0 and ws(300, 264, 48) == 0 and ws(300, 264, 31) == 0 and ws(300, 0, 32) == 0 and ws(300, (1 << 24) + 1, 32) == 0
    cfg = _cfg(CFG_1, 264)               # host-only: the rule with 256 CUs
    assert hra.lib.hrx_ctx_verify_chunk_rows(None, 8192, 32768) == 0
    for B, M in ((8192, 32768), (32768, 32768), (65536, 1024), (300, 264), (64, 2048), (1 << 20, 4096)):
        C = cfg.verify_chunk_rows(B, M)
        groups = (B + 63) // 64
        assert C % 64 == 0 and C > 0
        if groups >= 2048:
            assert C >= M, "enough strings for two waves a SIMD: one chunk"
        elif C < M:
            K = -(-M // C)
            assert C >= 256 and (groups * K >= 2048 or K == max(1, M // 256)) and (K == 1 or groups * (K - 1) < 2048)
    assert cfg.verify_chunk_rows(8192, 32768) == 2048 and cfg.verify_chunk_rows(1024, 32768) == 256 and cfg.verify_chunk_rows(65536, 1024) == 512
    assert cfg.verify_chunk_rows(300) >= 264


def test_refusals_of_the_host_entry():
    M = 64
    cfg = _cfg(CFG_1, M)
    chars, lens = synth.ragged(8, M, seed=1)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    want = cfg.verify_rows_host(chars, lens, rec, msk)
    long_lens = lens.copy()
    long_lens[3] = M + 1
    w = cfg.verify_rows_host(chars, long_lens, rec, msk, chunk_rows=32)
    assert w[3] == np.uint64(0xffffffffffffffff) and np.array_equal(np.delete(w, 3), np.delete(want, 3))
    out = np.full(8, 0x5555555555555555, np.uint64)
    args = (chars.ctypes.data, chars.shape[1], lens.ctypes.data, rec.ctypes.data, 0, msk.ctypes.data, 0, 8, M)
    f = hra.lib.hrx_verify_rows_chunked_host
    assert f(None, 0, *args, 32, out.ctypes.data) == hra.HRX_ERR_ARG
    assert f(cfg._ctx, 4, *args, 32, out.ctypes.data) == hra.HRX_ERR_ARG
    assert f(cfg._ctx, 0, *args, 32, out.ctypes.data + 4) == hra.HRX_ERR_ARG
    assert f(cfg._ctx, 0, *args[:4], M - 1, *args[5:], 32, out.ctypes.data) == hra.HRX_ERR_ARG      # pitch < M
    assert f(cfg._ctx, 0, *args[:8], (1 << 24) + 1, 32, out.ctypes.data) == hra.HRX_ERR_ARG
    for bad in (1, 31, 33, 48, 100):
        assert f(cfg._ctx, 0, *args, bad, out.ctypes.data) == hra.HRX_ERR_ARG                         # no multiple of 32
    assert (out == 0x5555555555555555).all()
    for C in (32, 64, 96, 1 << 30, 0):
        assert f(cfg._ctx, 0, *args, C, out.ctypes.data) == hra.HRX_OK and np.array_equal(out, want)
        out[:] = 0x5555555555555555
    # the device forms on a host-only context: no device; NULL ctx
    assert hra.lib.hrx_verify_rows_chunked_device(cfg._ctx, 0, 16, 16, 16, 16, 0, 16, 0, 8, M, 32, 16, 1 << 20, 16, None) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_verify_rows_chunked_device(None, 0, 16, 16, 16, 16, 0, 16, 0, 8, M, 32, 16, 1 << 20, 16, None) == hra.HRX_ERR_ARG
    assert np.array_equal(cfg.clone().verify_rows_host(chars, lens, rec, msk, chunk_rows=32), want)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_verify_chunk_host.cpp: the chunk walk (row by row and in every instantiation of the kernel's tile loop) and the fold against verify_string at
    M = 33, 64, 65, 139, 264 for every chunk_rows = 32, 64, 96, ... beyond M, events on both sides of every border, the summaries in a heap block of exactly
    hrx_verify_chunked_workspace_bytes, compiled with the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "hrx_test_verify_chunk_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_verify_chunk_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "verify chunk host: ok" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
