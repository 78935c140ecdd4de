"""ROUTE on the host (include/hrx.h: hrx_route_host behind route_host, no context): order / bucket_offsets against an expectation that never touches the code
under test — the oracle's status words (the batches of tests/test_extract_cpu.py), np.searchsorted(bounds, n, side="left") for the bucket and a stable
np.argsort for the order.  Padded (lens) and ragged (offsets) lengths, every require_accept, no screening, one to HRX_MAX_BUCKETS buckets, strings dropped
for length, decreasing offsets, guards behind both outputs, the argument rules, and the rules header as a program of its own under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import halo2_regex_amd as hra
from oracle_lib import ROOT
from test_extract_cpu import GUARD, batch, column

POISON64, POISON32 = np.uint64(0x5A5A5A5A5A5A5A5A), np.uint32(0x5A5A5A5A)
BATCHES = ["stress256", "lever256_second", "lever1001", "stress64_65537"]
EIGHT = [1, 15, 16, 17, 63, 64, 65]          # + [M]: HRX_MAX_BUCKETS bounds


def bounds_of(kind, M):
    """[M]; [16, 64, M]; HRX_MAX_BUCKETS bounds ending in M; [16, 64], below the longest string.  Bounds must increase strictly, so the batch of 64-row
    strings takes the lists with the same properties that fit it: [16, 32, 64], the eight bounds ending in 66, and [16, 32]"""
    if M == 64:
        return {"M": [64], "three": [16, 32, 64], "eight": EIGHT + [66], "short": [16, 32]}[kind]
    return {"M": [M], "three": [16, 64, M], "eight": EIGHT + [M], "short": [16, 64]}[kind]


def expect_route(status, n, valid, bounds, require_accept):
    """(order, bucket_offsets) as include/hrx.h ROUTE defines them: n the lengths (int64), valid False where a string has no length"""
    bounds = np.asarray(bounds, np.int64)
    keep = valid & (n <= bounds[-1])
    if status is not None:
        keep &= ((status & np.uint64(0xff)) == 0) & (((status >> np.uint64(8)) & np.uint64(require_accept)) == np.uint64(require_accept))
    bins = np.where(keep, np.searchsorted(bounds, n, side="left"), len(bounds))
    order = np.argsort(bins, kind="stable").astype(np.uint32)
    bo = np.concatenate((np.zeros(1, np.uint64), np.cumsum(np.bincount(bins, minlength=len(bounds) + 1), dtype=np.uint64)))
    return order, bo


def lengths_of(bt, form, lead=3):
    """the batch's lengths in one of the two forms -> (kwargs of route_host / route, n, valid)"""
    if form == "lens":
        return {"lens": bt.lens.astype(np.uint32)}, bt.lens.astype(np.int64), np.ones(len(bt.lens), bool)
    _, offsets = column(bt.chars, bt.lens, lead=lead)
    return {"offsets": offsets}, np.diff(offsets.astype(np.int64)), np.ones(len(bt.lens), bool)


def check_invariants(order, bo, B):
    assert np.array_equal(np.sort(order), np.arange(B, dtype=np.uint32))
    assert int(bo[0]) == 0 and int(bo[-1]) == B and (np.diff(bo.astype(np.int64)) >= 0).all()
    for j in range(len(bo) - 1):
        assert (np.diff(order[int(bo[j]):int(bo[j + 1])].astype(np.int64)) > 0).all(), j


def guarded(B, n_buckets):
    full = np.full(B + GUARD, POISON32), np.full(n_buckets + 2 + GUARD, POISON64)
    return (full[0][:B], full[1][:n_buckets + 2]), full


@pytest.mark.parametrize("form", ["lens", "offsets"])
@pytest.mark.parametrize("kind", ["M", "three", "eight", "short"])
@pytest.mark.parametrize("name", BATCHES)
def test_parity_with_numpy(name, kind, form):
    bt = batch(name)
    B, bounds = len(bt.lens), bounds_of(kind, bt.M)
    kw, n, valid = lengths_of(bt, form)
    for status, ra in ((bt.ost, 0), (bt.ost, 1), (bt.ost, 3), (None, 0)):
        out, full = guarded(B, len(bounds))
        r = hra.route_host(status, bounds=bounds, require_accept=ra, out=out, **kw)
        want = expect_route(status, n, valid, bounds, ra)
        assert np.array_equal(r.order, want[0]) and np.array_equal(r.bucket_offsets, want[1]), (name, kind, form, ra)
        check_invariants(r.order, r.bucket_offsets, B)
        assert (full[0][B:] == POISON32).all() and (full[1][len(bounds) + 2:] == POISON64).all()


def test_the_batches_hold_the_cases_they_are_chosen_for():
    """what the oracle and numpy say about the batches (nothing of the code under test): every accept mask, bad statuses, empty / one-element / large
    buckets, a mask that keeps nothing, strings dropped for length alone"""
    st = batch("stress256")
    assert not (st.ost & np.uint64(0xff)).any()
    assert np.bincount(((st.ost >> np.uint64(8)) & np.uint64(3)).astype(np.int64)).tolist() == [979, 508, 274, 239]
    n = st.lens.astype(np.int64)
    _, bo = expect_route(st.ost, n, np.ones(len(n), bool), EIGHT + [256], 1)
    assert np.diff(bo.astype(np.int64)).tolist() == [0, 0, 0, 0, 33, 1, 1, 712, 1253]
    for name in ("lever256_second", "lever1001"):
        codes = set((batch(name).ost & np.uint64(0xff)).tolist())
        assert {1, 2} <= codes, (name, codes)
    lv = batch("lever256_second")
    _, bo = expect_route(lv.ost, lv.lens.astype(np.int64), np.ones(len(lv.lens), bool), [256], 3)
    assert bo.tolist() == [0, 0, len(lv.lens)]                       # require_accept = 3 keeps nothing there
    _, bo = expect_route(None, n, np.ones(len(n), bool), [16, 64], 0)
    assert 0 < int(bo[2]) < len(n)                                    # [16, 64]: longer strings are dropped for length


def test_decreasing_offsets_are_dropped():
    offsets = np.array([3, 13, 9, 9, 80, 70, 71, 400], np.uint64)      # lengths 10, -, 0, 71, -, 1, 329
    status = np.array([1 << 8] * 7, np.uint64)
    n = np.array([10, 0, 0, 71, 0, 1, 329], np.int64)
    valid = np.array([1, 0, 1, 1, 0, 1, 1], bool)
    for bounds in ([16, 64, 256], [1024], [1, 10, 71]):
        r = hra.route_host(status, offsets=offsets, bounds=bounds, require_accept=1)
        want = expect_route(status, n, valid, bounds, 1)
        assert np.array_equal(r.order, want[0]) and np.array_equal(r.bucket_offsets, want[1])
        dropped = r.order[int(r.bucket_offsets[-2]):].tolist()
        assert 1 in dropped and 4 in dropped
    r = hra.route_host(None, offsets=offsets, bounds=[1, 10, 71])
    assert r.order.tolist() == [2, 5, 0, 3, 1, 4, 6] and r.bucket_offsets.tolist() == [0, 2, 3, 4, 7]      # n == bounds[j] belongs to bucket j


@pytest.mark.parametrize("B", [0, 1])
def test_tiny_batches(B):
    bt = batch("stress256").prefix(B)
    for form in ("lens", "offsets"):
        kw, n, valid = lengths_of(bt, form)
        out, full = guarded(B, 3)
        r = hra.route_host(bt.ost, bounds=[16, 64, 256], out=out, **kw)
        want = expect_route(bt.ost, n, valid, [16, 64, 256], 0)
        assert np.array_equal(r.order, want[0]) and np.array_equal(r.bucket_offsets, want[1])
        assert int(r.bucket_offsets[0]) == 0 and int(r.bucket_offsets[-1]) == B
        assert (full[0][B:] == POISON32).all() and (full[1][5:] == POISON64).all()


def _code(fn):
    with pytest.raises(hra.HrxError) as e:
        fn()
    return e.value.code


def test_argument_errors():
    bt = batch("stress256").prefix(8)
    lens = bt.lens.astype(np.uint32)
    _, offsets = column(bt.chars, bt.lens)
    assert _code(lambda: hra.route_host(bt.ost, lens=lens, offsets=offsets, bounds=[256])) == hra.HRX_ERR_ARG         # both
    assert _code(lambda: hra.route_host(bt.ost, bounds=[256])) == hra.HRX_ERR_ARG                                     # neither
    assert _code(lambda: hra.route_host(bt.ost, lens=lens, bounds=[])) == hra.HRX_ERR_ARG                             # n_buckets = 0
    assert _code(lambda: hra.route_host(bt.ost, lens=lens, bounds=list(range(1, 10)))) == hra.HRX_ERR_ARG             # n_buckets = 9
    assert _code(lambda: hra.route_host(bt.ost, lens=lens, bounds=[16, 16])) == hra.HRX_ERR_ARG                       # not increasing
    assert _code(lambda: hra.route_host(bt.ost, lens=lens, bounds=[64, 16])) == hra.HRX_ERR_ARG
    assert _code(lambda: hra.route_host(bt.ost, lens=lens, bounds=[16, (1 << 24) + 1])) == hra.HRX_ERR_ARG            # above 2^24
    hra.route_host(bt.ost, lens=lens, bounds=list(range(1, 9)))                                                      # HRX_MAX_BUCKETS of them, and ...
    hra.route_host(bt.ost, lens=lens, bounds=[1 << 24])                                                              # ... 2^24 itself are fine
    assert hra.MAX_BUCKETS == 8


def test_device_forms_on_a_host_only_context():
    """argument errors come first, then HRX_ERR_HIP: there is no device to launch on"""
    bt = batch("stress256").prefix(8)
    cfg = bt.make_cfg()
    lens, st = bt.lens.astype(np.uint32), bt.ost
    bounds = np.array([16, 64, 256], np.uint32)
    order, bo = np.zeros(8, np.uint32), np.zeros(5, np.uint64)
    ws = np.zeros(hra.route_workspace_bytes(8) // 8, np.uint64)
    import ctypes as C
    bp = bounds.ctypes.data_as(C.POINTER(C.c_uint32))
    args = (st.ctypes.data, 0, lens.ctypes.data, None, 8, bp, 3, order.ctypes.data, bo.ctypes.data)
    assert hra.lib.hrx_route_device(cfg._ctx, *args, ws.ctypes.data, ws.nbytes - 8, None) == hra.HRX_ERR_ARG          # workspace too small
    assert hra.lib.hrx_route_device(cfg._ctx, *args, ws.ctypes.data, ws.nbytes, None) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_route_device(None, *args, ws.ctypes.data, ws.nbytes, None) == hra.HRX_ERR_ARG
    assert hra.route_workspace_bytes(0) >= 72 and hra.route_workspace_bytes(1 << 20) < (1 << 20)
    chars = np.ascontiguousarray(bt.chars)
    pm, lo = np.zeros(8 * 256, np.uint8), np.zeros(8, np.uint32)
    sel = np.arange(8, dtype=np.uint32)
    g = (chars.ctypes.data, chars.shape[1], lens.ctypes.data, None, 8, sel.ctypes.data, 8, 256, pm.ctypes.data, lo.ctypes.data, None)
    assert hra.lib.hrx_gather_to_position_major_device(cfg._ctx, hra.LAYOUT_STRING_MAJOR, *g) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_gather_to_position_major_device(cfg._ctx, hra.LAYOUT_INPUT_POSITION_MAJOR, *g) == hra.HRX_ERR_ARG
    assert hra.lib.hrx_gather_to_position_major_device(None, hra.LAYOUT_STRING_MAJOR, *g) == hra.HRX_ERR_ARG


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_route_host.cpp: csrc/hrx_route.hpp + csrc/hrx_route_host.cpp compiled into a program of their own with the address and
    undefined-behaviour sanitizers: every input and output a heap block of exactly its size (an element too far is an error there)"""
    exe = str(tmp_path / "hrx_test_route_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_route_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "route host: ok" in out.stdout, out.stdout + out.stderr
