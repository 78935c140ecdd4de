"""LOOKUP COMPRESS on the host (include/hrx.h hrx_lookup_compress_inputs_host / hrx_lookup_compress_table_host / hrx_fr_mul on host-only contexts;
csrc/hrx_compress.hpp, csrc/hrx_fr.h): the Montgomery product against Python integers; the cells against tests/compress_ref.py — table rows and cells from
the oracle, tuples as src/lib.rs writes them, the fold in Python integers — limb for limb, on rows produced by witness_batch_host in every host row form, for
challenges at the field's edges, shared and per string, Montgomery and canonical; the table's cells; the closure that ties counts, table and inputs
together; tampered rows; the contract; and the arithmetic and the rule as a program of its own under the sanitizers.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import halo2_regex_amd as hra
from halo2_regex_amd import synth
from compress_ref import CompressRef, R, MONT, MONT_INV, limbs_of, int_of
from oracle_lib import OracleDefs, ROOT
from test_lookup_cpu import SETS, small_batch, to_position_major
from test_match_cpu import CFG_A, _cfg

_rng = np.random.default_rng(20)
T_RANDOM = int.from_bytes(_rng.bytes(32), "little") % R
THETAS = [0, 1, R - 1, T_RANDOM, T_RANDOM + R, (1 << 256) - 1]       # (T_RANDOM + r < 2 r < 2^256)
POISON = 0x5A5A5A5A5A5A5A5A


def theta_limbs(values):
    return np.array([limbs_of(v) for v in values], np.uint64)


# ---- hrx_fr_mul ---------------------------------------------------------------------------------------------------------------------------------
def mont_mul(a, b):
    return a * b * MONT_INV % R


def test_fr_mul_against_python_integers():
    edge = [0, 1, R - 1, MONT, MONT * MONT % R]
    rng = np.random.default_rng(7)
    pairs = [(a, b) for a in edge for b in edge] + [(int.from_bytes(rng.bytes(32), "little") % R, int.from_bytes(rng.bytes(32), "little") % R) for _ in range(200)]
    for a, b in pairs:
        got = int_of(hra.fr_mul(limbs_of(a), limbs_of(b)))
        assert got == mont_mul(a, b), (hex(a), hex(b))
        assert got == int_of(hra.fr_mul(limbs_of(b), limbs_of(a)))
        assert int_of(hra.fr_mul(limbs_of(a), limbs_of(MONT))) == a            # R is the Montgomery form of 1
    # of Montgomery forms the Montgomery form of the product: F::from(6) * F::from(7) == F::from(42)
    assert hra.fr_mul(hra.fr_from_u64(6), hra.fr_from_u64(7)) == hra.fr_from_u64(42)
    assert hra.FR_LOOKUP_COLUMN_NAMES(2) == ["trans[0]", "start[0]", "end[0]", "trans[1]", "start[1]", "end[1]"] and hra.lib.hrx_lookup_num_columns(5) == 15


# ---- the host twin against the yardstick --------------------------------------------------------------------------------------------------------
def batch_with_a_long_string(cfg, M):
    """small_batch's strings (n = 0, 1, M - 1, M and ragged noise) and their rows, then one more string's lens set to M + 1: it has no rows"""
    chars, lens = small_batch(M)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    lens = lens.copy()
    lens[-1] = M + 1
    return chars, lens, rec, st


def ref_cells(ref, chars, lens, rec, M, thetas, canonical, strings=None):
    """[3 D][B][M][4] uint64 from the yardstick; thetas: one integer, or one per string"""
    B = len(lens)
    out = np.zeros((3 * ref.D, B, M, 4), np.uint64)
    for b in (range(B) if strings is None else strings):
        th = thetas if isinstance(thetas, int) else thetas[b]
        out[:, b] = ref.cells_of_records(chars[b], int(lens[b]), M, rec[b], th, canonical)
    return out


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8, 31, 32, 33, 64])
@pytest.mark.parametrize("name", list(SETS))
def test_host_twin_against_the_yardstick_in_every_row_form(oracle, name, M):
    cfg = _cfg(SETS[name], M)
    ref = CompressRef(OracleDefs.from_files(oracle, SETS[name]))
    chars, lens, rec, st = batch_with_a_long_string(cfg, M)
    B, D = len(lens), cfg.num_defs
    assert {0, min(1, M), M - 1, M, M + 1} <= set(int(n) for n in lens)
    per_string = [THETAS[(b + b // len(THETAS)) % len(THETAS)] for b in range(B)]
    rp = np.full((B, M + 40, D), 0xffffffff, np.uint32)
    rp[:, :M] = rec
    rec_pm = to_position_major(rec, M, D)
    chars_pm = hra.chars_to_position_major(chars)
    PM, PM_IN = hra.LAYOUT_POSITION_MAJOR, hra.LAYOUT_POSITION_MAJOR | hra.LAYOUT_INPUT_POSITION_MAJOR
    for canonical in (False, True):
        want = ref_cells(ref, chars, lens, rec, M, per_string, canonical)
        th = theta_limbs(per_string)
        got = cfg.lookup_compress_inputs_host(chars, lens, rec, th, canonical=canonical)
        assert got.shape == (3 * D, B, M, 4) and np.array_equal(got, want), (name, M, canonical, np.argwhere(got != want)[:1])
        assert not got[:, -1].any()                                # n = M + 1: zero cells
        # a pitched view, the position-major image, position-major input: the same limbs
        assert np.array_equal(cfg.lookup_compress_inputs_host(chars, lens, rp[:, :M], th, canonical=canonical), got)
        assert np.array_equal(cfg.lookup_compress_inputs_host(chars, lens, rec_pm, th, layout=PM, canonical=canonical), got)
        assert np.array_equal(cfg.lookup_compress_inputs_host(chars_pm, lens, rec_pm, th, layout=PM_IN, chars_pm_stride=chars.shape[1], canonical=canonical), got)
        # one challenge for the whole call, each of the six; a window of it
        for t in THETAS:
            want = ref_cells(ref, chars, lens, rec, M, t, canonical)
            got = cfg.lookup_compress_inputs_host(chars, lens, rec, theta_limbs([t])[0], canonical=canonical)
            assert np.array_equal(got, want), (name, M, canonical, hex(t))
        win = cfg.lookup_compress_inputs_host(chars_pm, lens, rec_pm, theta_limbs(per_string[2:B - 1]), layout=PM_IN, chars_pm_stride=chars.shape[1],
                                              b_begin=2, b_count=B - 3, canonical=canonical)
        assert np.array_equal(win, ref_cells(ref, chars, lens, rec, M, per_string, canonical)[:, 2:B - 1])


def test_fold_at_the_top_of_its_range():
    """records with every bit of the id and both flags set and states within 1024 of 0xffff, under bytes within 4 of 0xff: every component about as large
    as a record can make it, 64 x 64 different rows, a challenge per string (r - 1 first) — the sums where the fold's quotient estimate is most often one
    short, against Python integers"""
    from compress_ref import cell_limbs, fold, theta_value
    M = B = 64
    cfg = _cfg(SETS["regex1"], M)
    dm = int(cfg.load()[0][0][0][1])
    idx = np.arange(B * M).reshape(B, M)
    chars = (0xff - idx % 4).astype(np.uint8)
    state = 0xffff - (idx * 7) % 1024
    lens = np.full(B, M, np.uint32)
    rec = (np.uint32(0xffff0000) | state.astype(np.uint32)).reshape(B, M, 1)
    rng = np.random.default_rng(11)
    vals = [R - 1] + [int.from_bytes(rng.bytes(32), "little") for _ in range(B - 1)]
    for canonical in (False, True):
        got = cfg.lookup_compress_inputs_host(chars, lens, rec, theta_limbs(vals), canonical=canonical)
        for b in range(B):
            th = theta_value(vals[b], canonical)
            for r in range(M):
                cur, nxt, c = int(state[b, r]), int(state[b, r + 1]) if r + 1 < M else dm, int(chars[b, r])
                for k, t in enumerate(((c, cur, nxt, 0xff), (0xff, cur, dm), (0xff, dm, nxt))):
                    assert got[k, b, r].tolist() == cell_limbs(fold(t, th), canonical), (b, r, k, canonical)


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_table_cells_against_the_yardstick(oracle, name):
    cfg = _cfg(SETS[name], 64)
    ref = CompressRef(OracleDefs.from_files(oracle, SETS[name]))
    W, lay = cfg.lookup_words(), cfg.lookup_layout()
    assert W == ref.words() and lay == ref.layout()
    used = lay[-1]["end"].stop
    for canonical in (False, True):
        got = cfg.lookup_compress_table_host(theta_limbs(THETAS), canonical=canonical)
        assert got.shape == (len(THETAS), W, 4)
        for k, t in enumerate(THETAS):
            assert np.array_equal(got[k], ref.table_cells(t, canonical)), (name, canonical, hex(t))
            assert not got[k, used:].any()                                           # the pad words
            for l in lay:
                assert np.array_equal(got[k, l["start"]], got[k, l["end"]])          # the two endpoint runs hold equal cells
        one = cfg.lookup_compress_table_host(theta_limbs([T_RANDOM])[0], canonical=canonical)
        assert one.shape == (1, W, 4) and np.array_equal(one[0], got[3])
    # a clone folds from tuples of its own
    assert np.array_equal(cfg.clone().lookup_compress_table_host(theta_limbs(THETAS), canonical=True), got)


# ---- counts, table and inputs tied together -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["regex12", "headers4"])
def test_closure_of_counts_table_and_inputs(oracle, name):
    """untampered rows, a random challenge: every input cell equals the table cell at the word the yardstick's hit gives, and per lookup the sorted multiset
    of the input cells equals the table cells repeated counts[w] times (counts from lookup_counts_host; at n == M the two cells of row M - 1 set aside)"""
    M = 33
    cfg = _cfg(SETS[name], M)
    ref = CompressRef(OracleDefs.from_files(oracle, SETS[name]))
    chars, lens = small_batch(M)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    clean = [b for b in range(len(lens)) if int(st[b]) & 0xff == 0]
    assert len(clean) >= 4 and any(int(lens[b]) == M for b in clean)
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    for canonical in (False, True):
        cells = cfg.lookup_compress_inputs_host(chars, lens, rec, theta_limbs([T_RANDOM])[0], canonical=canonical)
        table = cfg.lookup_compress_table_host(theta_limbs([T_RANDOM])[0], canonical=canonical)[0]
        for b in clean:
            n = int(lens[b])
            assert misses[b] == 0
            tuples = ref.tuples_of_string(bytes(chars[b, :n]), M)
            for d, lay in enumerate(cfg.lookup_layout()):
                for k, lk in enumerate(("trans", "start", "end")):
                    rows = M - 1 if n == M and k != 1 else M                 # row M - 1's transition and end lookups read the cell nobody assigns
                    for r in range(rows):
                        w = ref.hit(d, k, tuples[d][k][r])
                        assert w is not None and np.array_equal(cells[3 * d + k, b, r], table[w]), (b, d, lk, r)
                    got = sorted(tuple(int(v) for v in c) for c in cells[3 * d + k, b, :rows])
                    want = sorted(tuple(int(v) for v in c) for c in np.repeat(table[lay[lk]], counts[b][lay[lk]], axis=0))
                    assert got == want, (b, d, lk)


# ---- tampered rows ------------------------------------------------------------------------------------------------------------------------------
def tampered_rows(rec, n, M):
    """(name, rows) per mutation of one string's records (M, D): states, ids, flags, values outside every table — the list test_lookup_cpu.py judges the
    counts with, written out again"""
    u = np.uint32
    muts = {
        "state": lambda r: r.__setitem__((10, 0), (r[10, 0] & u(0xffff0000)) | u(3)),
        "sid": lambda r: r.__setitem__((3, 0), r[3, 0] | u(1 << 16)),
        "start": lambda r: r.__setitem__((22, 0), r[22, 0] | u(1 << 24)),
        "end_ok": lambda r: r.__setitem__((21, 0), r[21, 0] | u(1 << 25)),
        "end_bad": lambda r: r.__setitem__((20, 0), r[20, 0] | u(1 << 25)),
        "drop_start": lambda r: r.__setitem__((21, 0), r[21, 0] & ~u(1 << 24)),
        "pad_state": lambda r: r.__setitem__((100, 0), u(0)),
        "pad_flag": lambda r: r.__setitem__((M - 1, 1), r[M - 1, 1] | u(3 << 24)),
        "big_state": lambda r: r.__setitem__((5, 1), r[5, 1] | u(0xffff)),
        "big_state_pad": lambda r: r.__setitem__((n + 3, 0), r[n + 3, 0] | u(0xffff)),
        "big_sid": lambda r: r.__setitem__((7, 0), r[7, 0] | u(0xff << 16) | u(1 << 24)),
        "big_flags": lambda r: r.__setitem__((9, 1), r[9, 1] | u(0xfc << 24)),
        "all_ones": lambda r: r.__setitem__((30, slice(None)), u(0xffffffff)),
    }
    out = []
    for name, fn in muts.items():
        r = rec.copy()
        fn(r)
        out.append((name, r))
    return out


def test_tampered_rows_fold_as_they_lie_and_leave_the_table(oracle):
    M = 128
    s = b"email was meant for @yajk. Also for swq."
    n = len(s)
    cfg = _cfg(CFG_A, M)
    ref = CompressRef(OracleDefs.from_files(oracle, CFG_A))
    base = np.zeros((1, 48), np.uint8)
    base[0, :n] = np.frombuffer(s, np.uint8)
    rec0, msk0, st0 = cfg.witness_batch_host(base, np.array([n], np.uint32))
    cases = [("clean", rec0[0])] + tampered_rows(rec0[0], n, M)
    B = len(cases)
    chars, lens = np.repeat(base, B, 0), np.full(B, n, np.uint32)
    rec = np.stack([r for _, r in cases])
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    th = theta_limbs([T_RANDOM])[0]
    cells = cfg.lookup_compress_inputs_host(chars, lens, rec, th)
    table = cfg.lookup_compress_table_host(th)[0]
    lay = cfg.lookup_layout()
    in_run = [[{tuple(int(v) for v in c) for c in table[lay[d][lk]]} for lk in ("trans", "start", "end")] for d in range(2)]
    absent_in = set()
    for b, (name, _) in enumerate(cases):
        assert np.array_equal(cells[:, b], ref.cells_of_records(chars[b], n, M, rec[b], T_RANDOM, False)), name
        tuples = ref.tuples_of_records(chars[b], n, M, rec[b])
        missed = 0
        for d in range(2):
            for k in range(3):
                for r in range(M):
                    absent = tuple(int(v) for v in cells[3 * d + k, b, r]) not in in_run[d][k]
                    assert absent == (ref.hit(d, k, tuples[d][k][r]) is None), (name, d, k, r)
                    missed += absent
                    if absent:
                        absent_in.add(name)
        assert missed == int(misses[b]), name                      # (n < M: every lookup exists, so misses counts exactly the absent cells)
    assert absent_in == {"state", "sid", "start", "end_bad", "big_state", "big_sid", "all_ones"}


# ---- the contract -------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    M, B = 64, 24
    cfg = _cfg(CFG_A, M)
    D = cfg.num_defs
    chars, lens = synth.ragged(B, M, seed=1)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    G, n = 512, 3 * D * B * M * 4
    raw = np.full(G + n + G, POISON, np.uint64)
    out = raw[G:G + n]
    th = theta_limbs([T_RANDOM] * B)
    f, ctx = hra.lib.hrx_lookup_compress_inputs_host, cfg._ctx
    rows = (chars.ctypes.data, chars.shape[1], lens.ctypes.data, rec.ctypes.data, 0, B, M)
    ok = lambda *a: f(ctx, 0, *rows, 0, B, th.ctypes.data, 4, out.ctypes.data, 0)
    assert f(ctx, 0, *rows, 0, B, th.ctypes.data, 1, out.ctypes.data, 0) == hra.HRX_ERR_ARG                       # theta_stride not in {0, 4}
    assert f(ctx, 0, *rows, 0, B, th.ctypes.data, 8, out.ctypes.data, 0) == hra.HRX_ERR_ARG
    assert f(ctx, 0, *rows, 0, B, th.ctypes.data, 4, out.ctypes.data + 8, 0) == hra.HRX_ERR_ARG                   # cells not 16-byte aligned
    assert f(ctx, 0, *rows, 0, B, th.ctypes.data + 4, 4, out.ctypes.data, 0) == hra.HRX_ERR_ARG                   # theta not 8-byte aligned
    assert f(ctx, 0, *rows, 1, B, th.ctypes.data, 4, out.ctypes.data, 0) == hra.HRX_ERR_ARG                       # a window behind the batch
    assert f(ctx, 0, *rows, B + 1, 0, th.ctypes.data, 4, out.ctypes.data, 0) == hra.HRX_OK                        # (an empty window: no work)
    assert f(ctx, 0, *rows, 0, B, th.ctypes.data, 4, out.ctypes.data, 2) == hra.HRX_ERR_ARG                       # unknown flag bits
    assert f(ctx, 0, *rows, 0, B, th.ctypes.data, 4, out.ctypes.data, -1) == hra.HRX_ERR_ARG
    assert f(ctx, 4, *rows, 0, B, th.ctypes.data, 4, out.ctypes.data, 0) == hra.HRX_ERR_ARG                       # unknown layout
    assert f(ctx, 0, *rows[:4], M - 1, *rows[5:], 0, B, th.ctypes.data, 4, out.ctypes.data, 0) == hra.HRX_ERR_ARG  # pitch < M
    assert f(ctx, 0, *rows, 0, B, None, 4, out.ctypes.data, 0) == hra.HRX_ERR_ARG
    assert f(ctx, 0, *rows, 0, B, th.ctypes.data, 4, None, 0) == hra.HRX_ERR_ARG
    assert f(None, 0, *rows, 0, B, th.ctypes.data, 4, out.ctypes.data, 0) == hra.HRX_ERR_ARG
    # planes with a string-major layout; the device forms on a host-only context
    arr = (C.c_void_p * 2)(16, 16)
    g = hra.lib.hrx_lookup_compress_inputs_device_planes
    assert g(ctx, 0, 16, 16, 16, arr, 2, B, M, 0, B, 16, 4, 16, 0, None) == hra.HRX_ERR_ARG
    assert g(ctx, hra.LAYOUT_POSITION_MAJOR, 16, 16, 16, arr, 2, B, M, 0, B, 16, 4, 16, 0, None) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_lookup_compress_inputs_device(ctx, 0, 16, 16, 16, 16, 0, B, M, 0, B, 16, 4, 16, 0, None) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_lookup_compress_table_device(ctx, 16, 4, 1, 16, 0, None) == hra.HRX_ERR_HIP
    t = hra.lib.hrx_lookup_compress_table_host
    assert t(ctx, th.ctypes.data, 2, 3, out.ctypes.data, 0) == hra.HRX_ERR_ARG
    assert t(ctx, th.ctypes.data, 4, 3, out.ctypes.data + 8, 0) == hra.HRX_ERR_ARG
    assert t(ctx, th.ctypes.data + 4, 4, 3, out.ctypes.data, 0) == hra.HRX_ERR_ARG
    assert t(ctx, th.ctypes.data, 4, 3, out.ctypes.data, 4) == hra.HRX_ERR_ARG
    assert t(ctx, th.ctypes.data, 4, 1 << 16, out.ctypes.data, 0) == hra.HRX_ERR_ARG
    assert t(None, th.ctypes.data, 4, 3, out.ctypes.data, 0) == hra.HRX_ERR_ARG
    assert (raw == POISON).all()
    # the call they all are variations of writes its cells and nothing beside them; so does a window
    assert ok() == hra.HRX_OK and (raw[:G] == POISON).all() and (raw[G + n:] == POISON).all() and not (out == POISON).any()
    want = out.reshape(3 * D, B, M, 4).copy()
    raw[:] = POISON
    w = raw[G:G + 3 * D * 5 * M * 4].reshape(3 * D, 5, M, 4)
    got = cfg.lookup_compress_inputs_host(chars, lens, rec, th[7:12], b_begin=7, b_count=5, out=w)
    assert np.array_equal(got, want[:, 7:12]) and (raw[:G] == POISON).all() and (raw[G + w.size:] == POISON).all()
    with pytest.raises(hra.HrxError):
        cfg.lookup_compress_inputs_host(chars, lens, rec, th[:5])                      # theta of another shape than (B, 4) or (4,)


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_compress_host.cpp: csrc/hrx_fr.h + csrc/hrx_compress.hpp + csrc/hrx_compress_host.cpp compiled into a program of their own with
    the address and undefined-behaviour sanitizers — fr_mul and fr_add against a schoolbook product and binary long division, the fold at its extremes, the
    per-string loop over hand-made rows in heap blocks of exact size"""
    exe = str(tmp_path / "hrx_test_compress_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_compress_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "compress host: ok" in out.stdout, out.stdout + out.stderr
