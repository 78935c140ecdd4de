"""VERIFY on the host (include/hrx.h hrx_verify_rows_host on host-only contexts; csrc/hrx_verify.hpp): the verdict word's check bits against the torch checker
(tests/mock_prover.py, the definition of the bits) on the inputs of tests/test_mock_prover.py — the reference's own test inputs, its tamper list, the reveal
stress and ragged batches on the four def sets, the six random DFAs — on every string, whatever its status word says; the row field against the mutated row;
and the rules as a program of their own under the sanitizers.  No device."""
import os
import subprocess

import numpy as np
import pytest
import torch

import halo2_regex_amd as hra
from halo2_regex_amd import synth
from mock_prover import (IntegerMockProver, NAMES, VERIFY_BITS, FAIL_ACCEPT, FAIL_TRANSITION, FAIL_FIRST_STATE, FAIL_START_LOOKUP, FAIL_END_LOOKUP, FAIL_FLAGS,
                         FAIL_PADDING, FAIL_MASK, FAIL_ENABLE)
from oracle_lib import OracleDefs, ROOT, reference_cases
from test_mock_prover import CFG_1, CFG_3, CFG_A, CFG_123, _cfg, _verify

LOW = np.uint64(0xffffffff)


def bits_rows(v):
    return (v & LOW).astype(np.int64), (v >> np.uint64(32)).astype(np.int64)


def test_constants_are_the_checkers():
    assert (hra.VERIFY_FIRST_STATE, hra.VERIFY_ENABLE, hra.VERIFY_TRANSITION, hra.VERIFY_START_LOOKUP, hra.VERIFY_END_LOOKUP, hra.VERIFY_ACCEPT, hra.VERIFY_FLAGS,
            hra.VERIFY_PADDING, hra.VERIFY_MASK) == (FAIL_FIRST_STATE, FAIL_ENABLE, FAIL_TRANSITION, FAIL_START_LOOKUP, FAIL_END_LOOKUP, FAIL_ACCEPT, FAIL_FLAGS,
                                                     FAIL_PADDING, FAIL_MASK)
    assert hra.VERIFY_CIRCUIT_BITS == VERIFY_BITS and hra.VERIFY_NAMES == NAMES
    hdr = open(os.path.join(ROOT, "include", "hrx.h")).read()
    for name, value in (("FIRST_STATE", 1), ("ENABLE", 2), ("TRANSITION", 4), ("START_LOOKUP", 8), ("END_LOOKUP", 16), ("ACCEPT", 32), ("FLAGS", 64), ("PADDING", 128),
                        ("MASK", 256), ("CIRCUIT_BITS", 63), ("ROW_SHIFT", 32)):
        assert "HRX_VERIFY_%s = %d" % (name, value) in hdr
    assert hra.explain_verdict(0) == "ok" and hra.verdict_row(0) == 0
    assert hra.explain_verdict(FAIL_ACCEPT | FAIL_MASK | 17 << 32) == "accept chain + masked rows at row 17" and hra.verdict_row(FAIL_MASK | 17 << 32) == 17
    assert hra.verdict_row(-1) is None and hra.explain_verdict(np.uint64(0xffffffffffffffff)) == "longer than max_chars_size"


@pytest.mark.parametrize("case", reference_cases(), ids=[c["name"] for c in reference_cases()])
def test_reference_tests_verify_exactly_where_mockprover_does(oracle, case):
    """src/lib.rs:1067-1470: 0 for the pass cases; every test_substr_fail* input breaks the accept chain alone, at the first disabled row"""
    M = case["max_chars_size"]
    s = case["input"].encode("latin-1")
    chars = np.zeros((1, (len(s) + 15) // 16 * 16 or 16), np.uint8)
    chars[0, :len(s)] = np.frombuffer(s, np.uint8)
    lens = np.array([len(s)], np.uint32)
    cfg = _cfg(case["defs"], M)
    for rec, msk, st in (cfg.witness_batch_host(chars, lens), OracleDefs.from_files(oracle, case["defs"]).witness_batch(chars, lens, M)):
        v = int(cfg.verify_rows_host(chars, lens, rec, msk)[0])
        assert v == (0 if case["verify_ok"] else FAIL_ACCEPT | len(s) << 32), hra.explain_verdict(v)


def test_every_tampered_cell_gives_the_checkers_bits_at_its_row():
    """the tamper list of tests/test_mock_prover.py: the bits are the torch checker's for every mutation, the row is the mutated one — or the one before it
    where the Rotation::next pair (r - 1, r) is what breaks"""
    M = 128
    s = b"email was meant for @yajk. Also for swq."
    n = len(s)
    chars = np.zeros((1, 48), np.uint8)
    chars[0, :n] = np.frombuffer(s, np.uint8)
    lens = np.array([n], np.uint32)
    cfg = _cfg(CFG_A, M)
    mp = IntegerMockProver.from_config(cfg)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    assert int(cfg.verify_rows_host(chars, lens, rec, msk)[0]) == 0

    def set_state(r, m): r[0, 10, 0] = (r[0, 10, 0] & np.uint32(0xffff0000)) | np.uint32(3)
    def first(r, m): r[0, 0, 1] = (r[0, 0, 1] & np.uint32(0xffff0000)) | np.uint32(1)
    def sid(r, m): r[0, 3, 0] |= np.uint32(1 << 16)
    def start(r, m): r[0, 22, 0] |= np.uint32(1 << 24)
    def end(r, m): r[0, 21, 0] |= np.uint32(1 << 25)
    def end_bad(r, m): r[0, 20, 0] |= np.uint32(1 << 25)
    def drop_start(r, m): r[0, 21, 0] &= ~np.uint32(1 << 24)
    def pad_state(r, m): r[0, 100, 0] = 0
    def accept(r, m): r[0, n, 0] = (r[0, n, 0] & np.uint32(0xffff0000)) | np.uint32(3)
    def mchar(r, m): m[0, 21] = 0
    def mextra(r, m): m[0, 5] = 0x0161
    # (mutation, the bit it must show, the row of the word)
    for fn, bit, row in ((set_state, FAIL_TRANSITION, 9), (first, FAIL_FIRST_STATE, 0), (sid, FAIL_TRANSITION, 3), (start, FAIL_START_LOOKUP, 22), (end, 0, 0),
                         (end_bad, FAIL_END_LOOKUP, 20), (drop_start, FAIL_FLAGS, 21), (pad_state, FAIL_PADDING, 100), (accept, FAIL_ACCEPT, n - 1), (mchar, FAIL_MASK, 21),
                         (mextra, FAIL_MASK, 5)):
        r, m = rec.copy(), msk.copy()
        fn(r, m)
        want = int(_verify(mp, chars, lens, r, m, M)[0])
        v = int(cfg.verify_rows_host(chars, lens, r, m)[0])
        assert v & 0xffffffff == want and want & bit == bit, (fn.__name__, hra.explain_verdict(v), mp.explain(want))
        assert v >> 32 == row and v >> 57 == 0, (fn.__name__, hra.explain_verdict(v))


@pytest.mark.parametrize("names", [CFG_1, CFG_3, CFG_A, CFG_123], ids=["r1", "r3", "r1r2", "r1r2r3"])
def test_stress_batches_get_the_checkers_bits_on_every_string(oracle, names):
    """reveal_stress and ragged batches (n = 0 and n = M among them), host walk and oracle rows: the bits equal IntegerMockProver.verify on EVERY string —
    also where the status word is not ok and the rows are whatever the walk left — and the row of an accept-chain failure is n"""
    M = 264
    cfg = _cfg(names, M)
    mp = IntegerMockProver.from_config(cfg)
    o = OracleDefs.from_files(oracle, names)
    for chars, lens in (synth.reveal_stress(300, 260, seed=5), synth.ragged(300, M, seed=7)):
        lens = lens.copy()
        lens[0], lens[1] = 0, min(M, chars.shape[1])
        for rec, msk, st in (cfg.witness_batch_host(chars, lens), o.witness_batch(chars, lens, M, threads=4)):
            code = _verify(mp, chars, lens, rec, msk, M)
            bits, rows = bits_rows(cfg.verify_rows_host(chars, lens, rec, msk))
            assert np.array_equal(bits, code)
            ok = (st & np.uint64(0xff)) == 0
            assert ok.sum() > 100
            assert (rows[code == 0] == 0).all() and (rows[ok & (code == FAIL_ACCEPT)] == lens[ok & (code == FAIL_ACCEPT)]).all()
            # a pitched view and the position-major image of the same rows: the same words
            v = cfg.verify_rows_host(chars, lens, rec, msk)
            rp, mk = np.zeros((300, M + 40, len(names)), np.uint32), np.zeros((300, M + 24), np.uint16)
            rp[:, :M], mk[:, :M] = rec, msk
            assert np.array_equal(cfg.verify_rows_host(chars, lens, rp[:, :M], mk[:, :M]), v)


def test_position_major_image_gives_the_same_words():
    M, B = 264, 300
    cfg = _cfg(CFG_A, M)
    chars, lens = synth.reveal_stress(B, 260, seed=5)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    msk[7, 40] ^= 0x0101
    v = cfg.verify_rows_host(chars, lens, rec, msk)
    q4, q8 = (M + 3) // 4, (M + 7) // 8
    r4 = np.zeros((B, q4 * 4, 2), np.uint32)
    r4[:, :M] = rec
    m8 = np.zeros((B, q8 * 8), np.uint16)
    m8[:, :M] = msk
    rec_pm = np.ascontiguousarray(r4.reshape(B, q4, 4, 2).transpose(1, 3, 0, 2)).reshape(-1)
    msk_pm = np.ascontiguousarray(m8.reshape(B, q8, 8).transpose(1, 0, 2)).reshape(-1)
    assert np.array_equal(cfg.verify_rows_host(chars, lens, rec_pm, msk_pm, layout=hra.LAYOUT_POSITION_MAJOR), v)
    stride = chars.shape[1]
    chars_pm = hra.chars_to_position_major(chars)
    assert np.array_equal(cfg.verify_rows_host(chars_pm, lens, rec_pm, msk_pm, layout=hra.LAYOUT_POSITION_MAJOR | hra.LAYOUT_INPUT_POSITION_MAJOR,
                                               chars_pm_stride=stride), v)
    assert int(v[7]) & FAIL_MASK and int(v[7]) >> 32 <= 40


def test_random_definitions():
    """random DFAs of 5 .. 300 states (256 and 300: tables beyond one byte of state): the bits equal the torch checker's on every string"""
    for seed in range(6):
        nstates = [5, 17, 40, 120, 256, 300][seed]
        allstr, sub = synth.random_dfa(nstates, seed=seed, total=True, n_substr_pairs=30)
        defs = [hra.RegexDefs(hra.AllstrRegexDef(allstr), [hra.SubstrRegexDef(sub)])]
        M = 200
        cfg = hra.RegexVerifyConfig.configure(M, defs, device=hra.HRX_DEVICE_NONE)
        mp = IntegerMockProver.from_config(cfg)
        chars, lens = synth.ragged(120, M, seed=seed, planted=False)
        rec, msk, st = cfg.witness_batch_host(chars, lens)
        code = _verify(mp, chars, lens, rec, msk, M)
        bits, rows = bits_rows(cfg.verify_rows_host(chars, lens, rec, msk))
        assert ((st & np.uint64(0xff)) == 0).sum() > 60
        assert np.array_equal(bits, code)
        # and with one state per string moved (big states included): still the checker's bits, the row the pair before the moved cell or the cell itself
        r2 = rec.copy()
        pos = np.minimum(lens.astype(np.int64) // 2 + 1, M - 1)
        r2[np.arange(120), pos, 0] ^= np.uint32(1)
        code = _verify(mp, chars, lens, r2, msk, M)
        bits, rows = bits_rows(cfg.verify_rows_host(chars, lens, r2, msk))
        assert np.array_equal(bits, code) and (code != 0).all()
        clean = (st & np.uint64(0xff)) == 0
        assert ((rows[clean] == pos[clean] - 1) | (rows[clean] == pos[clean]) | (rows[clean] == lens[clean])).all()


def test_contract_of_the_host_form():
    M = 64
    cfg = _cfg(CFG_1, M)
    chars, lens = synth.ragged(8, M, seed=1)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    v = cfg.verify_rows_host(chars, lens, rec, msk)
    long_lens = lens.copy()
    long_lens[3] = M + 1
    w = cfg.verify_rows_host(chars, long_lens, rec, msk)
    assert w[3] == np.uint64(0xffffffffffffffff) and np.array_equal(np.delete(w, 3), np.delete(v, 3))
    out = np.full(8, 0x5555555555555555, np.uint64)
    args = (chars.ctypes.data, chars.shape[1], lens.ctypes.data, rec.ctypes.data, 0, msk.ctypes.data, 0, 8, M)
    assert hra.lib.hrx_verify_rows_host(None, 0, *args, out.ctypes.data) == hra.HRX_ERR_ARG
    assert hra.lib.hrx_verify_rows_host(cfg._ctx, 4, *args, out.ctypes.data) == hra.HRX_ERR_ARG
    assert hra.lib.hrx_verify_rows_host(cfg._ctx, 0, *args, out.ctypes.data + 4) == hra.HRX_ERR_ARG
    assert hra.lib.hrx_verify_rows_host(cfg._ctx, 0, *args[:4], M - 1, *args[5:], out.ctypes.data) == hra.HRX_ERR_ARG      # pitch < M
    assert hra.lib.hrx_verify_rows_host(cfg._ctx, 0, *args[:8], (1 << 24) + 1, out.ctypes.data) == hra.HRX_ERR_ARG
    assert (out == 0x5555555555555555).all()
    # the device forms on a host-only context: no device
    assert hra.lib.hrx_verify_rows_device(cfg._ctx, 0, 16, 16, 16, 16, 0, 16, 0, 8, M, 16, None) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_verify_rows_device(None, 0, 16, 16, 16, 16, 0, 16, 0, 8, M, 16, None) == hra.HRX_ERR_ARG
    # a clone verifies with tables of its own
    c2 = cfg.clone()
    assert np.array_equal(c2.verify_rows_host(chars, lens, rec, msk), v)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_verify_host.cpp: csrc/hrx_verify.hpp + csrc/hrx_verify_host.cpp compiled into a program of their own with the address and
    undefined-behaviour sanitizers — hand-made rows at M = 1, 7, 64, 65, n = 0 .. M, every image of them, the kernel's tile loop on the host; states, tags and
    flags outside every table in one to five defs at M = 33, 64, 65, in every instantiation of the tile loop the kernel uses, the image a heap block of its exact size"""
    exe = str(tmp_path / "hrx_test_verify_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_verify_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "verify host: ok" in out.stdout, out.stdout + out.stderr
