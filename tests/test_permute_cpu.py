"""LOOKUP PERMUTE on the host (include/hrx.h hrx_lookup_permute_host on host-only contexts; csrc/hrx_permute.hpp): the index columns against
hra.permuted_lookup_columns — the numpy construction, which shares nothing with csrc/ — on counts from lookup_counts_host and on hand-made counts; halo2's
constraints over the gathered cells in Python integers mod r; the pitch and the contract; and the rule as a program of its own under the sanitizers.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import halo2_regex_amd as hra
from compress_ref import R, int_of, limbs_of
from oracle_lib import ROOT
from test_lookup_cpu import SETS, small_batch
from test_match_cpu import CFG_23, CFG_A, _cfg

NAMES = ("trans", "start", "end")
NO_ROW = 0xffffffff
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def lookups_of(cfg):
    """[(column, slice into a string's run)] in hrx_lookup_num_columns' order"""
    return [(3 * d + k, lay[NAMES[k]]) for d, lay in enumerate(cfg.lookup_layout()) for k in range(3)]


def t_max(cfg):
    return max(sl.stop - sl.start for _, sl in lookups_of(cfg))


def check_against_numpy(cfg, counts, n_rows, res, strings=None):
    """the index columns of `res` (host or device arrays) against permuted_lookup_columns; an overflowing lookup against the overflow rule; returns the words"""
    a_idx, s_idx = np.asarray(res["a_idx"]).view(np.uint32), np.asarray(res["s_idx"]).view(np.uint32)
    over = np.zeros(len(counts), np.uint32)
    for b in (range(len(counts)) if strings is None else strings):
        for col, sl in lookups_of(cfg):
            m = counts[b][sl].astype(np.uint64)
            if int(m.sum(dtype=object)) > n_rows:
                over[b] |= np.uint32(1 << col)
                assert (a_idx[col, b, :n_rows] == NO_ROW).all() and (s_idx[col, b, :n_rows] == NO_ROW).all(), (b, col)
                continue
            A, S = hra.permuted_lookup_columns(sl.stop - sl.start, m, n_rows)
            assert np.array_equal(a_idx[col, b, :n_rows].astype(np.int64) - sl.start, A), (b, col, n_rows)
            assert np.array_equal(s_idx[col, b, :n_rows].astype(np.int64) - sl.start, S), (b, col, n_rows)
    return over


def hand_made_counts(cfg, n_rows):
    """one string per case, the case in the lookup with the longest table (T rows, n_rows >= T), (0, 2, 0, ...) in every other lookup; names and the bit of
    the long lookup where the case overflows"""
    # (beyond the issue's list: "a sum of 2^32", the case that tells a 32-bit sum from a 64-bit one)
    col, sl = max(lookups_of(cfg), key=lambda cs: cs[1].stop - cs[1].start)
    T, W = sl.stop - sl.start, cfg.lookup_words()
    cases = {
        "all zero": np.zeros(T, np.uint32),
        "every row once": np.ones(T, np.uint32) if n_rows == T else None,
        "one row holds everything": np.eye(1, T, T // 2, dtype=np.uint32)[0] * n_rows,
        "full without row 0": np.concatenate([[0], np.full(T - 1, (n_rows // (T - 1)), np.uint32)]) if T > 1 else None,
        "one too many": None,
        "two words of 0xffffffff": None,
        "a sum of 2^32": None,
    }
    if T > 1:
        full = cases["full without row 0"].astype(np.uint32)
        full[1::2] = 0                                      # every other row empty: a fill list with entries from all over the table
        full[-1] += n_rows - int(full.sum())                # sum == n_rows, m[0] == 0: row 0 heads the fill list
        cases["full without row 0"] = full
        cases["one too many"] = full.copy()
        cases["one too many"][T // 3 * 2] += 1
        big = np.zeros(T, np.uint32)
        big[[1, T - 1]] = 0xffffffff
        cases["two words of 0xffffffff"] = big
        wrap = np.zeros(T, np.uint32)                       # (two words of 0xffffffff wrap to 0xfffffffe, an overflow still: this sum wraps to 0)
        wrap[0], wrap[T - 1] = 0xffffffff, 1
        cases["a sum of 2^32"] = wrap
    cases = {k: v for k, v in cases.items() if v is not None}
    counts = np.zeros((len(cases), W), np.uint32)
    for c2, sl2 in lookups_of(cfg):
        if sl2.stop - sl2.start > 1:
            counts[:, sl2.start + 1] = 2
    for i, m in enumerate(cases.values()):
        counts[i, sl] = m
    want_over = np.array([(1 << col) if k in ("one too many", "two words of 0xffffffff", "a sum of 2^32") else 0 for k in cases], np.uint32)
    return list(cases), counts, want_over


# ---- the host twin against the yardstick --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 19, 64])
@pytest.mark.parametrize("name", list(SETS))
def test_host_twin_against_permuted_lookup_columns(name, M):
    cfg = _cfg(SETS[name], M)
    chars, lens = small_batch(M)
    assert {0, min(1, M), M - 1, M} <= set(int(n) for n in lens)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    base = max(M, t_max(cfg))
    for n_rows in (base, base + 1, (1 << base.bit_length()) - 6 if (1 << base.bit_length()) - 6 >= base else (2 << base.bit_length()) - 6):
        res = cfg.lookup_permute_host(counts, n_rows)
        assert res["a_idx"].shape == (3 * cfg.num_defs, len(lens), (n_rows + 3) & ~3)
        over = check_against_numpy(cfg, counts, n_rows, res)
        assert not over.any() and not res["overflow"].any()


@pytest.mark.parametrize("exact", [True, False])
def test_hand_made_counts(exact):
    cfg = _cfg(CFG_A, 8)
    n_rows = t_max(cfg) + (0 if exact else 37)
    names, counts, want_over = hand_made_counts(cfg, n_rows)
    assert ("every row once" in names) == exact and "full without row 0" in names
    table = cfg.lookup_compress_table_host(np.array(limbs_of(12345), np.uint64))[0]
    res = cfg.lookup_permute_host(counts, n_rows, table=table)
    over = check_against_numpy(cfg, counts, n_rows, res)
    assert np.array_equal(over, want_over) and np.array_equal(res["overflow"], want_over), names
    col, sl = max(lookups_of(cfg), key=lambda cs: cs[1].stop - cs[1].start)
    for i, k in enumerate(names):
        a, s = res["a_idx"][col, i, :n_rows], res["s_idx"][col, i, :n_rows]
        if want_over[i]:
            assert not res["a_cells"][col, i].any() and not res["s_cells"][col, i].any()
        else:
            assert np.array_equal(res["a_cells"][col, i, :n_rows], table[a]) and np.array_equal(res["s_cells"][col, i, :n_rows], table[s])
        if k == "every row once":                       # every position a first position, no fill
            assert np.array_equal(a, np.arange(sl.start, sl.stop)) and np.array_equal(s, a)
        if k == "full without row 0":
            first = np.r_[True, a[1:] != a[:-1]]
            assert a[0] == sl.start + 2 and s[~first][0] == sl.start, "row 0 heads the fill list"
        if k == "all zero":
            assert (a == sl.start).all() and s[0] == sl.start and np.array_equal(s[1:sl.stop - sl.start], np.arange(sl.start + 1, sl.stop))
    # the other lookups of an overflowing string are built as ever (check_against_numpy went over them); their cells too
    for c2, sl2 in lookups_of(cfg):
        if c2 != col:
            assert np.array_equal(res["a_cells"][c2, :, :n_rows], table[res["a_idx"][c2, :, :n_rows]])


# ---- halo2's constraints over the cells ---------------------------------------------------------------------------------------------------------
def as_ints(cells):
    return [int_of(c) for c in cells]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("per_string", [False, True])
def test_constraints_of_the_lookup_argument_over_the_cells(per_string, canonical):
    M = 19
    cfg = _cfg(CFG_23, M)
    chars, lens = small_batch(M)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    B, n_rows = len(lens), max(M, t_max(cfg)) + 3
    rng = np.random.default_rng(11)
    thetas = np.array([limbs_of(int.from_bytes(rng.bytes(32), "little") % R) for _ in range(B)], np.uint64)
    theta = thetas if per_string else thetas[0]
    table = cfg.lookup_compress_table_host(theta, canonical=canonical)
    inputs = cfg.lookup_compress_inputs_host(chars, lens, rec, theta, canonical=canonical)
    res = cfg.lookup_permute_host(counts, n_rows, table=table if per_string else table[0])
    assert not res["overflow"].any()
    clean = [b for b in range(B) if int(st[b]) & 0xff == 0 and misses[b] == 0]
    assert any(int(lens[b]) == M for b in clean) and any(int(lens[b]) < M for b in clean)
    for b in range(B):
        run = table[b if per_string else 0]
        for col, sl in lookups_of(cfg):
            T = sl.stop - sl.start
            A, S = as_ints(res["a_cells"][col, b, :n_rows]), as_ints(res["s_cells"][col, b, :n_rows])
            assert A[0] == S[0]
            assert all((A[i] - S[i]) * (A[i] - A[i - 1]) % R == 0 for i in range(1, n_rows)), (b, col)
            cell0 = int_of(run[sl.start])
            assert sorted(S) == sorted(as_ints(run[sl]) + [cell0] * (n_rows - T)), (b, col)
            if b in clean:
                inp = as_ints(inputs[col, b])
                if int(lens[b]) == M and col % 3 != 1:
                    inp[M - 1] = cell0              # the counts leave row M - 1's transition and end lookups out: the cell nobody assigns
                assert sorted(A) == sorted(inp + [cell0] * (n_rows - M)), (b, col)


# ---- layout and contract ------------------------------------------------------------------------------------------------------------------------
def test_pitch_tails_keep_their_poison():
    cfg = _cfg(CFG_23, 5)
    chars, lens = small_batch(5)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    counts, _ = cfg.lookup_counts_host(chars, lens, rec)
    B, ncols, n_rows = len(lens), 3 * cfg.num_defs, t_max(cfg) + 1
    table = cfg.lookup_compress_table_host(np.array(limbs_of(7), np.uint64))[0]
    want = cfg.lookup_permute_host(counts, n_rows, table=table)              # pitch = 0: n_rows rounded up
    p0 = (n_rows + 3) & ~3
    assert want["a_idx"].shape[2] == p0
    for pitch in (p0, p0 + 4, 1 << n_rows.bit_length()):
        out = {"a_idx": np.full((ncols, B, pitch), POISON32, np.uint32), "s_idx": np.full((ncols, B, pitch), POISON32, np.uint32),
               "a_cells": np.full((ncols, B, pitch, 4), POISON64, np.uint64), "s_cells": np.full((ncols, B, pitch, 4), POISON64, np.uint64)}
        res = cfg.lookup_permute_host(counts, n_rows, table=table, pitch=pitch, out=out)
        for k in out:
            assert np.array_equal(res[k][:, :, :n_rows], want[k][:, :, :n_rows]), (pitch, k)
            assert (res[k][:, :, n_rows:] == (POISON32 if "idx" in k else POISON64)).all(), (pitch, k)
    # indices only, cells only: the same words
    only = cfg.lookup_permute_host(counts, n_rows, out=("idx",))
    assert set(only) == {"a_idx", "s_idx", "overflow"} and np.array_equal(only["s_idx"], want["s_idx"])
    only = cfg.lookup_permute_host(counts, n_rows, table=table, out=("cells",), overflow=False)
    assert set(only) == {"a_cells", "s_cells"} and np.array_equal(only["a_cells"], want["a_cells"])


def test_refused_calls_write_nothing():
    cfg = _cfg(CFG_23, 5)
    W, ncols, T = cfg.lookup_words(), 3 * cfg.num_defs, t_max(cfg)
    B, n_rows = 2, T + 2
    pitch = (n_rows + 3) & ~3
    counts = np.zeros((B, W), np.uint32)
    table = np.zeros((W, 4), np.uint64)
    # 16 bytes of slack in front of each output, so that a pointer 4 bytes further is misaligned and still inside
    ai, si = (np.full(ncols * B * pitch + 4, POISON32, np.uint32) for _ in range(2))
    ac, sc = (np.full(ncols * B * pitch * 4 + 2, POISON64, np.uint64) for _ in range(2))
    ov = np.full(B + 1, POISON32, np.uint32)
    f, ctx = hra.lib.hrx_lookup_permute_host, cfg._ctx
    P = lambda a, off=0: a.ctypes.data + off
    good = dict(counts=P(counts), b_count=B, n_rows=n_rows, pitch=pitch, a_idx=P(ai), s_idx=P(si), table=P(table), stride=0, a_cells=P(ac), s_cells=P(sc), ov=P(ov))

    def call(**kw):
        a = dict(good, **kw)
        return f(ctx, a["counts"], a["b_count"], a["n_rows"], a["pitch"], a["a_idx"], a["s_idx"], a["table"], a["stride"], a["a_cells"], a["s_cells"], a["ov"])

    bad = [dict(n_rows=T - 1, pitch=0), dict(n_rows=(1 << 24) + 1, pitch=0), dict(pitch=pitch + 2), dict(pitch=pitch - 4), dict(stride=4), dict(stride=4 * W + 4),
           dict(s_idx=None), dict(a_idx=None), dict(table=None), dict(a_cells=None), dict(s_cells=None), dict(a_idx=None, s_idx=None, table=None, a_cells=None, s_cells=None),
           dict(counts=None), dict(counts=P(counts, 4)), dict(a_idx=P(ai, 4)), dict(s_idx=P(si, 8)), dict(table=P(table, 8)), dict(a_cells=P(ac, 8)), dict(s_cells=P(sc, 8)),
           dict(ov=P(ov, 2))]
    for kw in bad:
        assert call(**kw) == hra.HRX_ERR_ARG, kw
        assert (ai == POISON32).all() and (si == POISON32).all() and (ac == POISON64).all() and (sc == POISON64).all() and (ov == POISON32).all(), kw
    assert f(None, *[good[k] for k in ("counts", "b_count", "n_rows", "pitch", "a_idx", "s_idx", "table", "stride", "a_cells", "s_cells", "ov")]) == hra.HRX_ERR_ARG
    assert call(b_count=0) == hra.HRX_OK and (ai == POISON32).all()
    assert call() == hra.HRX_OK and call(stride=4 * W, table=P(np.zeros((B, W, 4), np.uint64))) == hra.HRX_OK and call(pitch=0) == hra.HRX_OK
    assert (ai[:ncols * B * pitch].reshape(ncols, B, pitch)[:, :, :n_rows] != POISON32).all() and (ov[:B] == 0).all() and ov[B] == POISON32
    # the device form on a host-only context: the argument rules first, then HRX_ERR_HIP
    g = hra.lib.hrx_lookup_permute_device
    args = [good[k] for k in ("counts", "b_count", "n_rows", "pitch", "a_idx", "s_idx", "table", "stride", "a_cells", "s_cells", "ov")]
    assert g(ctx, *args, None, 0, None) == hra.HRX_ERR_HIP
    assert cfg.lookup_permute_workspace_bytes(B, n_rows) == 0
    plan = cfg.lookup_permute_plan(B, n_rows)
    assert plan["group_rows"] % plan["tile_rows"] == 0 and plan["groups"] * plan["group_rows"] >= n_rows and plan["chunk_rows"] >= 1


def test_workspace_only_for_tables_beyond_a_chunk():
    from halo2_regex_amd import synth
    a_txt, sub_txt = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=200)
    cfg = hra.RegexVerifyConfig.configure(64, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub_txt)])], device=hra.HRX_DEVICE_NONE)
    T, W = t_max(cfg), cfg.lookup_words()
    plan = cfg.lookup_permute_plan(2, T)
    assert T == 65537 and T > plan["chunk_rows"] and plan["groups"] == 1
    assert cfg.lookup_permute_workspace_bytes(2, T) == 2 * W * 4
    # the host twin on that table: uniform counts, and one bin holding nearly all
    counts = np.zeros((2, W), np.uint32)
    sl = cfg.lookup_layout()[0]["trans"]
    counts[0, sl.start:sl.stop:2] = 2
    counts[1, sl.start + 40000] = T - 5
    counts[1, sl.start + 7] = 3
    for n_rows in (T, T + 63):
        check_against_numpy(cfg, counts, n_rows, cfg.lookup_permute_host(counts, n_rows))


# ---- the rule under the sanitizers --------------------------------------------------------------------------------------------------------------
def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_permute_host.cpp: csrc/hrx_permute.hpp + csrc/hrx_permute_host.cpp compiled into a program of their own with the address and
    undefined-behaviour sanitizers — random and hand-made counts against a literal transcription of the rule, every buffer a heap block of its exact size"""
    exe = str(tmp_path / "hrx_test_permute_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_permute_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "permute host: ok" in out.stdout, out.stdout + out.stderr
