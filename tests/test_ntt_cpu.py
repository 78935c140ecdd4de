"""FR NTT on the host (include/hrx.h hrx_fr_ntt_host / hrx_ctx_fr_ntt_plan / hrx_fr_sub on host-only contexts; csrc/hrx_ntt.hpp): the host twin against
ntt_ref — Python integers, the two sums transcribed — limb for limb: every size from 2 to 256 against the naive sums, 2^10, 2^12, 2^13 against an independent
iterative transform, 2^16 by Horner evaluation; both directions and limb forms, the shifts, n_in with the unread entries poisoned, pitches, in place, the
refusals, and the rule as a program of its own under the sanitizers.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import halo2_regex_amd as hra
import ntt_ref as nr
from compress_ref import R, MONT, cell_limbs, int_of, limbs_of
from oracle_lib import ROOT
from test_match_cpu import CFG_1, _cfg

POISON64 = 0x5A5A5A5A5A5A5A5A
CFG = None


def cfg():
    global CFG
    if CFG is None:
        CFG = _cfg(CFG_1, 64)
    return CFG


def elements(count, seed):
    """seeded field elements; the first three are 0, 1 and r - 1"""
    rng = np.random.default_rng(seed)
    return ([0, 1, R - 1] + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(max(count - 3, 0))])[:count]


def columns(n_cols, n_in, pitch, seed, canonical):
    """(values [n_cols][n_in], cells [n_cols][pitch][4] with every entry from n_in on poisoned)"""
    vals = [elements(n_in, seed + 97 * c)[::-1] if c & 1 else elements(n_in, seed + 97 * c) for c in range(n_cols)]
    cells = np.full((n_cols, pitch, 4), POISON64, np.uint64)
    for c in range(n_cols):
        cells[c, :n_in] = nr.cells_of(vals[c], canonical)
    return vals, cells


def shift_limbs(g, canonical):
    return None if g is None else np.array(cell_limbs(g, canonical), np.uint64)


def check(k, inverse, canonical, g, n_in, n_cols, ref, seed=3, out_pitch=None, in_place=False):
    n = 1 << k
    out_pitch = out_pitch or (n + 3) & ~3
    in_pitch = out_pitch if in_place else (n_in + 3) & ~3
    vals, cells = columns(n_cols, n_in, in_pitch, seed, canonical)
    out = cells if in_place else np.full((n_cols, out_pitch, 4), POISON64, np.uint64)
    res = cfg().fr_ntt_host(cells, k, out=out, inverse=inverse, n_in=n_in, shift=shift_limbs(g, canonical), canonical=canonical)
    assert res is out
    for c in range(n_cols):
        want = ref(vals[c], k, inverse, 1 if g is None else g)
        assert np.array_equal(out[c, :n], nr.cells_of(want, canonical)), (k, inverse, canonical, g, n_in, c)
    assert (out[:, n:] == POISON64).all(), "entries above 2^k are never written"
    return vals, out


# ---- the constants and fr_sub ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_fields():
    assert hra.FR_S == nr.S == 28
    assert hra.FR_ROOT_OF_UNITY == nr.ROOT_OF_UNITY == pow(7, (R - 1) >> 28, R)
    assert pow(hra.FR_ROOT_OF_UNITY, 1 << 27, R) == R - 1 and pow(hra.FR_ROOT_OF_UNITY, 1 << 28, R) == 1
    for k in (1, 2, 24):
        assert pow(nr.omega(k), 1 << k, R) == 1 and pow(nr.omega(k), 1 << (k - 1), R) == R - 1


def test_fr_sub_against_python_integers():
    edge = [0, 1, R - 1, MONT, MONT * MONT % R, (R + 1) // 2]
    sample = edge + elements(40, 12)
    for a in sample:
        for b in edge + sample[-6:]:
            assert int_of(hra.fr_sub(limbs_of(a), limbs_of(b))) == (a - b) % R, (a, b)
    assert int_of(hra.fr_sub(limbs_of(5 + R), limbs_of(7))) == R - 2           # taken mod r first
    assert hra.fr_sub(hra.fr_from_u64(50), hra.fr_from_u64(8)) == hra.fr_from_u64(42)


# ---- the transform against the yardstick --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("k", range(1, 9))
def test_host_twin_against_the_naive_sums(k, inverse, canonical):
    g = elements(5, 40 + k)[4]
    check(k, inverse, canonical, g, 1 << k, 3 if k < 8 else 1, nr.naive, seed=k)
    if k <= 6:
        check(k, inverse, canonical, None, 1 << k, 2, nr.naive, seed=k + 20)


@pytest.mark.parametrize("k,inverse,canonical", [(10, False, False), (10, True, True), (12, True, False), (12, False, True), (13, False, False), (13, True, False)])
def test_host_twin_against_the_iterative_transform(k, inverse, canonical):
    assert nr.iterative(elements(16, 1), 4, inverse, 7) == nr.naive(elements(16, 1), 4, inverse, 7)      # the two yardsticks agree
    check(k, inverse, canonical, 7, 1 << k, 2, nr.iterative, seed=k)
    check(k, inverse, canonical, None, 1 << (k - 2), 1, nr.iterative, seed=k + 1)


def test_size_2_to_the_16_by_horner():
    """lagrange_to_coeff: the inverse transform's output evaluated at w^i is entry i of the column"""
    k, n = 16, 1 << 16
    vals, cells = columns(2, n, n, 8, False)
    coeffs = cfg().fr_ntt_host(cells, k, inverse=True)
    w = nr.omega(k)
    for c in range(2):
        co = nr.values_of(coeffs[c], False)
        for i in (0, 1, 2, n // 2 - 1, n // 2, 12345, n - 2, n - 1):
            assert nr.eval_at(co, pow(w, i, R)) == vals[c][i], (c, i)


# ---- the argument forms ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
def test_shifts_and_the_round_trip_through_a_coset(canonical):
    k, n = 5, 32
    for g in (None, 1, 7, nr.ZETA, elements(4, 77)[3]):
        vals, fwd = check(k, False, canonical, g, n, 3, nr.naive)
        ginv = None if g is None else pow(g, -1, R)
        back = cfg().fr_ntt_host(fwd, k, inverse=True, shift=shift_limbs(ginv, canonical), canonical=canonical)
        for c in range(3):
            assert np.array_equal(back[c], nr.cells_of(vals[c], canonical)), g
    _, one = check(k, False, canonical, 1, n, 1, nr.naive)
    _, none = check(k, False, canonical, None, n, 1, nr.naive)
    assert np.array_equal(one, none)
    unreduced = np.array(limbs_of(cell_limbs_int(7, canonical) + R), np.uint64)           # taken mod r first
    vals, cells = columns(1, n, n, 3, canonical)
    assert np.array_equal(cfg().fr_ntt_host(cells, k, shift=unreduced, canonical=canonical)[0], nr.cells_of(nr.naive(vals[0], k, False, 7), canonical))


def cell_limbs_int(v, canonical):
    return int_of(cell_limbs(v, canonical))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("k", [2, 6])
def test_n_in_pitches_columns_and_in_place(k, inverse):
    n = 1 << k
    for n_in in sorted({1, 2, n - 1, n, n >> 2}):
        check(k, inverse, False, 7, n_in, 3, nr.naive)
        check(k, inverse, True, None, n_in, 2, nr.naive, in_place=True, out_pitch=n + 8)
    for n_cols in (1, 3, 17):
        check(k, inverse, False, nr.ZETA, n, n_cols, nr.naive, out_pitch=n + 4)
        check(k, inverse, False, nr.ZETA, n >> 2, n_cols, nr.naive, in_place=True)


def test_inverse_of_forward_is_the_identity_and_a_unit_vector_gives_powers():
    for k in (1, 3, 7, 11):
        n = 1 << k
        vals, cells = columns(2, n, max(n, 4), k, False)                                  # (k = 1: the smallest pitch is 4)
        fwd = cfg().fr_ntt_host(cells, k, n_in=n)
        assert np.array_equal(cfg().fr_ntt_host(fwd, k, inverse=True, n_in=n)[:, :n], cells[:, :n])
        assert np.array_equal(cfg().fr_ntt_host(cfg().fr_ntt_host(cells, k, inverse=True, n_in=n), k, n_in=n)[:, :n], cells[:, :n])
    k, n, g = 6, 64, 7
    for pos in (0, 1, 5, n - 1):
        unit = nr.cells_of([1 if i == pos else 0 for i in range(n)], False)
        got = nr.values_of(cfg().fr_ntt_host(unit, k, shift=shift_limbs(g, False)), False)
        assert got == [pow(g, pos, R) * pow(nr.omega(k), pos * j, R) % R for j in range(n)]
    constant = nr.values_of(cfg().fr_ntt_host(nr.cells_of([R - 1] * n, True), k, inverse=True, canonical=True), True)
    assert constant == [R - 1] + [0] * (n - 1)
    assert not cfg().fr_ntt_host(np.zeros((n, 4), np.uint64), k).any()


def test_python_shapes():
    k, n = 4, 16
    vals, cells = columns(3, n, n, 1, False)
    one = cfg().fr_ntt_host(cells[1], k)
    assert one.shape == (n, 4) and np.array_equal(one, cfg().fr_ntt_host(cells, k)[1])
    assert cfg().fr_ntt_host(cells[:, :4].copy(), k).shape == (3, n, 4)                   # n_in = in_pitch = 4
    for bad in (dict(out=np.zeros((2, n, 4), np.uint64)), dict(out=np.zeros((3, n, 4), np.uint32)), dict(shift=np.zeros((2, 4), np.uint64))):
        with pytest.raises(hra.HrxError) as e:
            cfg().fr_ntt_host(cells, k, **bad)
        assert e.value.code == hra.HRX_ERR_ARG
    with pytest.raises(hra.HrxError):
        cfg().fr_ntt_host(cells, 25)


# ---- the plan and the contract ----------------------------------------------------------------------------------------------------------------------------
def test_plan_covers_every_size():
    one_pass = [k for k in range(1, 25) if cfg().fr_ntt_plan(1, k)["n_passes"] == 1]
    assert one_pass == list(range(1, one_pass[-1] + 1)) and one_pass[-1] >= 10
    for k in range(1, 25):
        p = cfg().fr_ntt_plan(5, k)
        assert 1 <= p["n_passes"] <= 3 and sum(p["pass_bits"]) == k and all(b >= 1 for b in p["pass_bits"])
        assert p["cols_per_group"] >= 1 and (p["cols_per_group"] == 1 or p["n_passes"] == 1)
        assert hra.lib.hrx_fr_ntt_workspace_bytes(k) >= 32 * ((1 << k) // 2 + 1) and hra.lib.hrx_fr_ntt_workspace_bytes(k) % 256 == 0
    assert cfg().fr_ntt_workspace_bytes(0) == 0 and cfg().fr_ntt_workspace_bytes(25) == 0
    with pytest.raises(hra.HrxError):
        cfg().fr_ntt_plan(1, 0)


def aligned(n_bytes, align=256, fill=0x5A):
    raw = np.full(n_bytes + align, fill, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw, raw[off:off + n_bytes]


def test_refusals_write_nothing_and_a_host_only_context_has_no_device_form():
    k, n, ctx = 4, 16, cfg()._need_ctx()
    _, inb = aligned(3 * 32 * n * 2)
    raw, outb = aligned(3 * 32 * n * 2)
    _, shift = aligned(32)
    inp, outp, sp = inb.ctypes.data, outb.ctypes.data, shift.ctypes.data
    INV, CAN = hra.FR_NTT_INVERSE, hra.FR_CANONICAL
    host = lambda *a: hra.lib.hrx_fr_ntt_host(ctx, *a)
    good = (inp, n, outp, n, 3, k, n, sp, 0)
    inb[:] = 0
    shift[:] = 0
    assert host(*good) == hra.HRX_OK
    outb[:] = 0x5A
    bad = {
        "NULL in": (None, n, outp, n, 3, k, n, sp, 0), "NULL out": (inp, n, None, n, 3, k, n, sp, 0),
        "misaligned in": (inp + 8, n, outp, n, 3, k, n, sp, 0), "misaligned out": (inp, n, outp + 8, n, 3, k, n, sp, 0),
        "misaligned shift": (inp, n, outp, n, 3, k, n, sp + 4, 0),
        "k = 0": (inp, n, outp, n, 3, 0, 1, sp, 0), "k = 25": (inp, n, outp, n, 3, 25, n, sp, 0),
        "n_in = 0": (inp, n, outp, n, 3, k, 0, sp, 0), "n_in above 2^k": (inp, n + 4, outp, n + 4, 3, k, n + 1, sp, 0),
        "in_pitch below n_in": (inp, n - 4, outp, n, 3, k, n, sp, 0), "in_pitch no multiple of 4": (inp, n + 2, outp, n, 3, k, n, sp, 0),
        "out_pitch below 2^k": (inp, n, outp, n - 4, 3, k, n - 4, sp, 0), "out_pitch no multiple of 4": (inp, n, outp, n + 1, 3, k, n, sp, 0),
        "unknown flag": (inp, n, outp, n, 3, k, n, sp, 4), "unknown flags": (inp, n, outp, n, 3, k, n, sp, INV | CAN | 8),
        "overlap, shifted": (outp + 32, n, outp, n, 3, k, n, sp, 0), "overlap, other pitch": (outp, n, outp, n + 4, 3, k, n, sp, 0),
        "overlap, out inside in": (outp, n, outp + 32 * n, n, 3, k, n, sp, 0),
    }
    for what, args in bad.items():
        assert host(*args) == hra.HRX_ERR_ARG, what
        assert (raw == 0x5A).all(), what
    assert host(outp, n, outp, n, 3, k, n >> 1, None, INV | CAN) == hra.HRX_OK             # in place, and no shift, are fine
    assert host(inp, n, outp, n, 0, 99, 0, None, 77) == hra.HRX_OK                          # no columns: nothing to check, nothing done
    # the device forms: the same refusals first, then the context has no device
    _, ws = aligned(hra.lib.hrx_fr_ntt_workspace_bytes(k))
    wp, wb = ws.ctypes.data, ws.size
    dev = lambda *a: hra.lib.hrx_fr_ntt_device(ctx, *a)
    outb[:] = 0x5A
    for what, args in bad.items():
        assert dev(*args, wp, wb, None) == hra.HRX_ERR_ARG, what
    for what, w in {"no workspace": (None, wb), "misaligned workspace": (wp + 128, wb), "small workspace": (wp, wb - 1)}.items():
        assert dev(*good, *w, None) == hra.HRX_ERR_ARG, what
        assert hra.lib.hrx_fr_ntt_prepare_device(ctx, k, *w, None) == hra.HRX_ERR_ARG, what
    assert hra.lib.hrx_fr_ntt_prepare_device(ctx, 0, wp, wb, None) == hra.HRX_ERR_ARG
    assert dev(*good, wp, wb, None) == hra.HRX_ERR_HIP
    assert hra.lib.hrx_fr_ntt_prepare_device(ctx, k, wp, wb, None) == hra.HRX_ERR_HIP
    assert dev(inp, n, outp, n, 0, k, n, sp, 0, wp, wb, None) == hra.HRX_OK
    assert (raw == 0x5A).all() and (ws == 0x5A).all()


# ---- the rule under the sanitizers --------------------------------------------------------------------------------------------------------------
def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_ntt_host.cpp: csrc/hrx_fr.h + csrc/hrx_ntt.hpp + csrc/hrx_ntt_host.cpp compiled into a program of their own with the address and
    undefined-behaviour sanitizers — the host twin at k <= 6 against the two sums over a schoolbook product, every buffer a heap block of its exact size"""
    exe = str(tmp_path / "hrx_test_ntt_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_ntt_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ntt host: ok" in out.stdout, out.stdout + out.stderr
