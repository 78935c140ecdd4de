"""LOOKUP QUOTIENT on the host (include/hrx.h hrx_fr_vanishing_inverse_host / hrx_lookup_quotient_host / hrx_ctx_lookup_quotient_plan on host-only
contexts; csrc/hrx_quotient.hpp): the host twin against quotient_ref — Python integers, the five steps as they are written — limb for limb:
  sizes            every (k, e) with k in 1..6 and e in 1..3 (N below rot x 64 and k = 1 among them), 3 D = 3 and 3 D = 6, 1 and 3 strings
  argument forms   both limb forms, challenges per string and per call, s_stride 0 and 1, h_in NULL, separate and in place, four different pitches with
                   the tails poisoned and found intact, the inputs unchanged, with and without HRX_QUOTIENT_DIVIDE; cells of 0, 1, r - 1; unreduced challenges
  the table        the vanishing inverse for g in {7, ZETA, ZETA^2, 1}; the selectors against direct evaluation of the Lagrange bases
  refusals         every one, with nothing written; a host-only context has no device form
  the chain        regex1 at M = 64 through counts, compress, permute, invert, product, the transforms to the coset of ZETA at k = 14, the quotient: the
                   reference at every point, h is zero modulo X^n - 1, the divided q has degree below 3 n and h = (X^n - 1) q; a tampered Z breaks it
and the rule as a program of its own under the sanitizers.  No device."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import halo2_regex_amd as hra
import ntt_ref as nr
import quotient_ref as qr
from compress_ref import R, cell_limbs, int_of, limbs_of
from oracle_lib import ROOT
from test_match_cpu import CFG_1, CFG_23, _cfg
from test_ntt_cpu import aligned, elements
from test_product_cpu import Chain, batch

POISON64 = 0x5A5A5A5A5A5A5A5A
SIZES = [(k, e) for k in range(1, 7) for e in range(1, 4)]
H_MODES = ("none", "separate", "in place")
_CFGS = {}


def cfg_of(ncols):
    """a host-only context with ncols = 3 D lookups: regex1, or regex2 + regex3"""
    if ncols not in _CFGS:
        _CFGS[ncols] = _cfg({3: CFG_1, 6: CFG_23}[ncols], 64)
    return _CFGS[ncols]


def shift_limbs(g, canonical):
    return np.array(cell_limbs(g, canonical), np.uint64)


class Case:
    """seeded inputs of one call in numpy arrays of four different pitches, the tails poisoned; the integers they stand for; the reference"""

    def __init__(self, ncols, k, e, b_count, canonical=False, per_string=False, s_stride=0, h_mode="none", divide=False, seed=1, unreduced=False):
        self.ncols, self.k, self.ext_k, self.b_count, self.canonical, self.h_mode, self.divide = ncols, k, k + e, b_count, canonical, h_mode, divide
        N = self.N = 1 << (k + e)
        self.pitch, self.s_pitch, self.sel_pitch, self.h_pitch = N + 4, N + 8, N + 12, N + 16
        runs = b_count if s_stride else 1
        draw = itertools.count(seed * 1000)

        def column():
            v = elements(N, next(draw))
            return v[::-1] if next(draw) & 1 else v                                     # 0, 1, r - 1 at either end

        def cells(shape, pitch, vals):
            out = np.full(shape + (pitch, 4), POISON64, np.uint64)
            for idx in np.ndindex(*shape):
                out[idx][:N] = nr.cells_of(vals[idx], canonical)
            return out

        self.vals = {name: {idx: column() for idx in np.ndindex(ncols, b_count)} for name in ("A", "Ap", "Sp", "Z")}
        self.vals["S"] = {idx: column() for idx in np.ndindex(ncols, runs)}
        self.sel_vals = {(i,): column() for i in range(3)}
        self.arrays = {name: cells((ncols, b_count), self.pitch, self.vals[name]) for name in ("A", "Ap", "Sp", "Z")}
        self.arrays["S"] = cells((ncols, runs), self.s_pitch, self.vals["S"])
        if not s_stride:
            self.arrays["S"] = self.arrays["S"][:, 0]
        self.arrays["sel"] = cells((3,), self.sel_pitch, self.sel_vals)
        n_ch = b_count if per_string else 1
        ch = [elements(3 + n_ch, next(draw))[3:] for _ in range(3)]                    # beta, gamma, y
        self.ch_vals = [[c[b if per_string else 0] for b in range(b_count)] for c in ch]
        lim = lambda v: limbs_of(int_of(cell_limbs(v, canonical)) + (R if unreduced else 0))      # (below 2 r < 2^256; taken mod r first)
        self.challenges = [np.array([lim(v) for v in c], np.uint64) if per_string else np.array(lim(c[0]), np.uint64) for c in ch]
        self.h_vals = {(b,): column() for b in range(b_count)} if h_mode != "none" else None
        self.h_in = cells((b_count,), self.h_pitch, self.h_vals) if self.h_vals else None
        self.g = 7
        self.t_vals = qr.t_inv(k, k + e, self.g)
        self.t_inv = nr.cells_of(self.t_vals, canonical) if divide else None

    def want(self, b):
        """the reference cells of string b: [N][4]"""
        runs = lambda c: self.vals["S"][(c, b if (c, b) in self.vals["S"] else 0)]
        lookups = [{"A": self.vals["A"][(c, b)], "Ap": self.vals["Ap"][(c, b)], "Sp": self.vals["Sp"][(c, b)], "Z": self.vals["Z"][(c, b)], "S": runs(c)}
                   for c in range(self.ncols)]
        beta, gamma, y = (c[b] for c in self.ch_vals)
        out = qr.fold(self.k, self.ext_k, lookups, tuple(self.sel_vals[(i,)] for i in range(3)), beta, gamma, y,
                      self.h_vals[(b,)] if self.h_vals else None, self.t_vals if self.divide else None)
        return nr.cells_of(out, self.canonical)

    def call_args(self, arrays=None, h_in=None, out=None):
        a = arrays or self.arrays
        return dict(k=self.k, ext_k=self.ext_k, a_ext=a["A"], ap_ext=a["Ap"], sp_ext=a["Sp"], z_ext=a["Z"], s_ext=a["S"], selectors=a["sel"],
                    beta=self.challenges[0], gamma=self.challenges[1], y=self.challenges[2], h_in=h_in, out=out, t_inv=self.t_inv, divide=self.divide,
                    canonical=self.canonical)

    def run_host(self):
        """the host twin on this case: the reference at every point, the pitch tails and the inputs as they were"""
        keep = {name: a.copy() for name, a in self.arrays.items()}
        h_keep = None if self.h_in is None else self.h_in.copy()
        if self.h_mode == "in place":
            h_in = out = self.h_in.copy()
        else:
            h_in, out = self.h_in, np.full((self.b_count, self.h_pitch, 4), POISON64, np.uint64)
        res = cfg_of(self.ncols).lookup_quotient_host(**self.call_args(h_in=h_in, out=out))
        assert res is out
        for b in range(self.b_count):
            assert np.array_equal(out[b, :self.N], self.want(b)), (self.k, self.ext_k, b)
        tail = h_keep[:, self.N:] if self.h_mode == "in place" else POISON64
        assert (out[:, self.N:] == tail).all(), "entries above 2^ext_k are never written"
        assert all(np.array_equal(self.arrays[name], keep[name]) for name in keep) and (h_keep is None or np.array_equal(self.h_in, h_keep)), "no input is written"
        return out


# ---- the host twin against the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,ke", list(enumerate(SIZES)))
def test_host_twin_at_every_size(i, ke):
    """every (k, e); the argument forms turn with the size so that each appears at small and large N, and every size sees both limb forms"""
    k, e = ke
    for canonical in (False, True):
        j = i + (1 if canonical else 0)
        Case(3, k, e, 1 + 2 * (j & 1), canonical, per_string=bool(j & 2), s_stride=(j >> 2) & 1, h_mode=H_MODES[j % 3], divide=bool((j >> 1) & 1), seed=i + 1).run_host()
    if e == 2:
        Case(6, k, e, 3 if k < 5 else 1, canonical=bool(k & 1), per_string=True, s_stride=1, h_mode=H_MODES[k % 3], divide=True, seed=40 + k).run_host()


@pytest.mark.parametrize("canonical", [False, True])
def test_every_argument_form_at_one_size(canonical):
    seed = 100
    for per_string, s_stride, h_mode, divide in itertools.product((False, True), (0, 1), H_MODES, (False, True)):
        seed += 1
        Case(3, 3, 2, 3, canonical, per_string, s_stride, h_mode, divide, seed).run_host()
    Case(6, 2, 1, 3, canonical, True, 0, "separate", True, seed + 1).run_host()
    Case(6, 1, 3, 1, canonical, False, 1, "in place", False, seed + 2).run_host()


@pytest.mark.parametrize("canonical", [False, True])
def test_unreduced_challenges_and_edge_cells(canonical):
    a = Case(3, 4, 1, 3, canonical, True, 1, "separate", True, seed=7)
    b = Case(3, 4, 1, 3, canonical, True, 1, "separate", True, seed=7, unreduced=True)
    assert not np.array_equal(a.challenges[0], b.challenges[0])
    assert np.array_equal(a.run_host(), b.run_host())
    # columns that are all 0, all 1, all r - 1: every product with a zero factor, the sums that wrap
    for v in (0, 1, R - 1):
        c = Case(3, 2, 2, 1, canonical, False, 0, "separate", True, seed=9)
        for name in ("A", "Ap", "Sp", "Z", "S"):
            for idx in c.vals[name]:
                c.vals[name][idx] = [v] * c.N
                c.arrays[name][idx[:c.arrays[name].ndim - 2]][:c.N] = cell_limbs(v, canonical)      # (one table run for the call: S has no string axis)
        c.run_host()


def test_python_shapes_and_the_plan():
    c = Case(3, 3, 1, 2, seed=3)
    cfg = cfg_of(3)
    out = cfg.lookup_quotient_host(**c.call_args())
    assert out.shape == (2, c.N, 4) and np.array_equal(out[1], c.want(1))                  # a fresh buffer of pitch 2^ext_k
    for bad in (dict(out=np.zeros((3, c.N, 4), np.uint64)), dict(h_in=np.zeros((2, c.N, 3), np.uint64)), dict(divide=True)):
        with pytest.raises(hra.HrxError) as err:
            cfg.lookup_quotient_host(**dict(c.call_args(), **bad))
        assert err.value.code == hra.HRX_ERR_ARG
    with pytest.raises(hra.HrxError):
        cfg_of(6).lookup_quotient_host(**c.call_args())                                    # three lookups' columns, six lookups' context
    assert hra.QUOTIENT_DIVIDE == 4
    for ext_k in (2, 8, 14, 24):
        p = cfg.lookup_quotient_plan(3, ext_k)
        assert p["tile_cells"] >= 64 and p["tile_cells"] % 64 == 0 and p["cells_per_lane"] >= 1 and p["tile_cells"] % p["cells_per_lane"] == 0
    with pytest.raises(hra.HrxError):
        cfg.lookup_quotient_plan(1, 25)


# ---- the vanishing inverse and the selectors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
def test_vanishing_inverse_against_python_integers(canonical):
    cfg = cfg_of(3)
    for k, e in [(1, 1), (1, 6), (3, 2), (6, 3), (12, 2), (18, 6), (23, 1)]:
        for g in (7, nr.ZETA, nr.ZETA * nr.ZETA % R, 1):
            got = cfg.fr_vanishing_inverse_host(k, k + e, shift_limbs(g, canonical), canonical=canonical)
            want = qr.t_inv(k, k + e, g)
            assert got.shape == (1 << e, 4) and np.array_equal(got, nr.cells_of(want, canonical)), (k, e, g)
            if g == 1:
                assert not got[0].any() and all(want[1:])                               # g in the subgroup: X^n - 1 is zero at c = 0, and only there
            xs = [(pow(g, 1 << k, R) * pow(nr.omega(k + e), (1 << k) * c, R) - 1) % R for c in range(1 << e)]
            assert all(v * x % R == (1 if x else 0) for v, x in zip(want, xs))
    assert np.array_equal(cfg.fr_vanishing_inverse_host(3, 5, None, canonical=canonical), cfg.fr_vanishing_inverse_host(3, 5, shift_limbs(1, canonical), canonical=canonical))
    unreduced = np.array(limbs_of(int_of(cell_limbs(7, canonical)) + R), np.uint64)
    assert np.array_equal(cfg.fr_vanishing_inverse_host(3, 5, unreduced, canonical=canonical), nr.cells_of(qr.t_inv(3, 5, 7), canonical))


def test_vanishing_inverse_with_g_one_is_zero_only_where_the_denominator_is():
    """g = 1: the coset is the extended subgroup itself, X^n - 1 vanishes at c = 0 (and there the cell is zero); the issue's `every entry is zero` holds of the
    entries whose denominator is zero — quotient_ref has the rule, and the library follows it"""
    got = nr.values_of(cfg_of(3).fr_vanishing_inverse_host(2, 4, shift_limbs(1, True), canonical=True), True)
    assert got[0] == 0 and got == qr.t_inv(2, 4, 1)


@pytest.mark.parametrize("canonical", [False, True])
def test_selectors_against_direct_evaluation(canonical):
    cfg = cfg_of(3)
    for k, e, n_rows, g in [(1, 1, 1, 7), (2, 3, 2, nr.ZETA), (4, 2, 9, 7), (5, 1, 31, nr.ZETA * nr.ZETA % R), (6, 2, 0, 7)]:
        got = cfg.lookup_quotient_selectors(k, k + e, n_rows, shift_limbs(g, canonical), canonical=canonical)
        assert got.shape == (3, max(1 << (k + e), 4), 4)
        for i, want in enumerate(qr.selectors(k, k + e, n_rows, g)):
            assert np.array_equal(got[i, :1 << (k + e)], nr.cells_of(want, canonical)), (k, e, n_rows, i)
    with pytest.raises(hra.HrxError):
        cfg.lookup_quotient_selectors(3, 5, 8, shift_limbs(7, False))                      # row n_rows must exist


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def refusals(k, e, b, ncols, ptr):
    """every refused argument list of the quotient call (without ctx, and stream), by name, next to a good one; ptr: name -> address of a buffer large enough
    for pitch N + 16"""
    N = 1 << (k + e)
    p = N + 16
    good = [b, k, k + e, ptr["a"], ptr["ap"], ptr["sp"], ptr["z"], p, ptr["s"], p, 1, ptr["sel"], p, ptr["beta"], ptr["gamma"], ptr["y"], 4, ptr["h_in"], ptr["h_out"], p,
            ptr["t"], hra.QUOTIENT_DIVIDE]
    names = ["b_count", "k", "ext_k", "a", "ap", "sp", "z", "pitch", "s", "s_pitch", "s_stride", "sel", "sel_pitch", "beta", "gamma", "y", "challenge_stride", "h_in",
             "h_out", "h_pitch", "t_inv", "flags"]
    at = {n: i for i, n in enumerate(names)}

    def with_(**kw):
        a = list(good)
        for n, v in kw.items():
            a[at[n]] = v
        return tuple(a)

    bad = {}
    for n in ("a", "ap", "sp", "z", "s", "sel", "beta", "gamma", "y", "h_out"):
        bad["NULL " + n] = with_(**{n: None})
    for n in ("a", "ap", "sp", "z", "s", "sel", "h_in", "h_out", "t_inv"):
        bad["misaligned " + n] = with_(**{n: good[at[n]] + 8})
    for n in ("beta", "gamma", "y"):
        bad["misaligned " + n] = with_(**{n: good[at[n]] + 4})
    for n in ("pitch", "s_pitch", "sel_pitch", "h_pitch"):
        bad[n + " below 2^ext_k"] = with_(**{n: N - 4})
        bad[n + " no multiple of 4"] = with_(**{n: N + 2})
    bad.update({"k = 0": with_(k=0, ext_k=e), "e = 0": with_(ext_k=k), "e = 7": with_(k=1, ext_k=8), "ext_k below k": with_(ext_k=k - 1),
                "ext_k = 25": with_(k=24, ext_k=25), "s_stride 2": with_(s_stride=2), "s_stride 4": with_(s_stride=4), "challenge_stride 1": with_(challenge_stride=1),
                "challenge_stride 8": with_(challenge_stride=8), "divide without t_inv": with_(t_inv=None), "unknown flag": with_(flags=2),
                "unknown flags": with_(flags=hra.FR_CANONICAL | hra.QUOTIENT_DIVIDE | 8),
                "h_in shifted over h_out": with_(h_in=ptr["h_out"] + 32), "h_out inside z": with_(h_out=ptr["z"] + 32 * p), "h_out is a": with_(h_out=ptr["a"]),
                "h_out over the selectors": with_(h_out=ptr["sel"] + 64), "h_out over s": with_(h_out=ptr["s"]), "h_out over t_inv": with_(h_out=ptr["t"])})
    return tuple(good), bad, with_


def test_refusals_write_nothing_and_a_host_only_context_has_no_device_form():
    k, e, b, ncols = 3, 2, 2, 3
    N = 1 << (k + e)
    ctx = cfg_of(ncols)._need_ctx()
    size = ncols * b * (N + 16) * 32
    bufs = {n: aligned(size, fill=0) for n in ("a", "ap", "sp", "z", "s", "sel", "h_in", "t")}
    bufs.update({n: aligned(b * 32, fill=0) for n in ("beta", "gamma", "y")})
    bufs["h_out"] = aligned(size)
    ptr = {n: v[1].ctypes.data for n, v in bufs.items()}
    raw = bufs["h_out"][0]
    good, bad, with_ = refusals(k, e, b, ncols, ptr)
    host = lambda *a: hra.lib.hrx_lookup_quotient_host(ctx, *a)
    dev = lambda *a: hra.lib.hrx_lookup_quotient_device(ctx, *a, None)
    assert host(*good) == hra.HRX_OK and not (raw == 0x5A).all()
    assert host(*with_(h_in=None)) == hra.HRX_OK and host(*with_(h_in=ptr["h_out"])) == hra.HRX_OK      # no h_in, and in place, are fine
    assert host(*with_(t_inv=None, flags=0)) == hra.HRX_OK and host(*with_(t_inv=ptr["h_out"] + 8, flags=0)) == hra.HRX_OK      # t_inv is ignored without the flag
    raw[:] = 0x5A
    for what, args in bad.items():
        assert host(*args) == hra.HRX_ERR_ARG, what
        assert dev(*args) == hra.HRX_ERR_ARG, what
        assert (raw == 0x5A).all(), what
    assert hra.lib.hrx_lookup_quotient_host(None, *good) == hra.HRX_ERR_ARG
    assert host(*with_(b_count=0, k=99, flags=77)) == hra.HRX_OK and dev(*with_(b_count=0)) == hra.HRX_OK      # no strings: nothing to check, nothing done
    assert dev(*good) == hra.HRX_ERR_HIP and (raw == 0x5A).all()
    # the vanishing inverse
    traw, t = aligned(64 * 32)
    tp, sp = t.ctypes.data, ptr["beta"]
    vh = lambda *a: hra.lib.hrx_fr_vanishing_inverse_host(ctx, *a)
    for what, args in {"NULL t_inv": (k, k + e, sp, None, 0), "misaligned t_inv": (k, k + e, sp, tp + 8, 0), "misaligned shift": (k, k + e, sp + 4, tp, 0),
                       "k = 0": (0, e, sp, tp, 0), "e = 0": (k, k, sp, tp, 0), "e = 7": (k, k + 7, sp, tp, 0), "ext_k = 25": (24, 25, sp, tp, 0),
                       "unknown flag": (k, k + e, sp, tp, 2), "divide is no flag here": (k, k + e, sp, tp, hra.QUOTIENT_DIVIDE)}.items():
        assert vh(*args) == hra.HRX_ERR_ARG, what
        assert hra.lib.hrx_fr_vanishing_inverse_device(ctx, *args, None) == hra.HRX_ERR_ARG, what
        assert (traw == 0x5A).all(), what
    assert hra.lib.hrx_fr_vanishing_inverse_device(ctx, k, k + e, sp, tp, 0, None) == hra.HRX_ERR_HIP and (traw == 0x5A).all()
    assert vh(k, k + e, sp, tp, 0) == hra.HRX_OK and (t[(32 << e):] == 0x5A).all() and not (t[:(32 << e)] == 0x5A).all()      # 2^e entries and none above
    out = (hra.C.c_size_t * 2)()
    assert hra.lib.hrx_ctx_lookup_quotient_plan(None, 1, 8, out, out) == hra.HRX_ERR_ARG and hra.lib.hrx_ctx_lookup_quotient_plan(ctx, 1, 8, None, out) == hra.HRX_ERR_ARG


# ---- the chain, on the host ---------------------------------------------------------------------------------------------------------------------------
K, EXT_K, N_ROWS = 12, 14, 4090


def lagrange_columns(cfg, ch, z, seed, tamper=None):
    """A, S, A', S', Z of regex1's lookups in Lagrange form at pitch 2^12 — A[r] and S[r] by LOOKUP PRODUCT's definition, A' and S' gathered from the table
    through the index columns — with the rows above n_rows (Z: above n_rows + 1 entries) filled with seeded elements; tamper: (lookup, string, row) of a Z
    entry to change"""
    n, M, B, ncols = 1 << K, ch.M, ch.B, 3 * cfg.num_defs
    table = ch.table
    blind = nr.cells_of(elements(n, seed), ch.canonical)
    cols = {name: np.zeros((ncols, B, n, 4), np.uint64) for name in ("A", "Ap", "Sp", "Z")}
    S = np.zeros((ncols, n, 4), np.uint64)
    lay = cfg.lookup_layout()
    for c in range(ncols):
        sl = lay[c // 3][("trans", "start", "end")[c % 3]]
        off, T = sl.start, sl.stop - sl.start
        S[c, :T] = table[off:off + T]
        S[c, T:] = table[off]                                                           # S of the rows above n_rows too: the table column is fixed, not blinded
        for b in range(B):
            nb = int(ch.lens[b])
            A = cols["A"][c, b]
            A[:] = table[off]
            if nb <= M:
                rows = M - 1 if (nb == M and c % 3 != 1) else M
                A[:rows] = ch.inputs[c, b, :rows]
            cols["Ap"][c, b, :N_ROWS] = table[ch.a_idx[c, b, :N_ROWS]]
            cols["Sp"][c, b, :N_ROWS] = table[ch.s_idx[c, b, :N_ROWS]]
            cols["Z"][c, b, :N_ROWS + 1] = z[c, b, :N_ROWS + 1]
            for name in ("A", "Ap", "Sp"):
                cols[name][c, b, N_ROWS:] = blind[(c + b) % 7:][:n - N_ROWS]
            cols["Z"][c, b, N_ROWS + 1:] = blind[5:][:n - N_ROWS - 1]
    if tamper:
        c, b, r = tamper
        cols["Z"][c, b, r] = blind[3]
    return cols, S


def to_coset(cfg, lagrange, canonical, g):
    flat = lagrange.reshape(-1, 1 << K, 4)
    coeff = cfg.fr_ntt_host(flat, K, inverse=True, canonical=canonical)
    return cfg.fr_ntt_host(coeff, EXT_K, n_in=1 << K, shift=shift_limbs(g, canonical), canonical=canonical).reshape(lagrange.shape[:-2] + (1 << EXT_K, 4))


_CHAIN = {}


def host_chain(canonical=False):
    """the host chain of regex1 at M = 64, once: the honest strings of test_product_cpu's batch, the columns on the coset of ZETA, the selectors, y"""
    if canonical not in _CHAIN:
        cfg = cfg_of(3)
        chars, lens, rec = batch(cfg)
        full = Chain(cfg, chars, lens, rec, N_ROWS, canonical, per_string=False, seed=21)
        keep = full.honest()[:3]
        assert len(keep) == 3
        ch = Chain(cfg, chars[keep], lens[keep], rec[keep], N_ROWS, canonical, per_string=False, seed=21)
        perm = cfg.lookup_permute_host(ch.counts, N_ROWS, pitch=1 << K, out=("idx",))      # idx pitch = z_pitch = 2^12
        ch.a_idx, ch.s_idx = perm["a_idx"], perm["s_idx"]
        z = ch.product(z_pitch=1 << K)["z"]
        assert tuple(ch.a_idx.shape) == (3, 3, 1 << K) and z.shape == (3, 3, 1 << K, 4)
        y = np.array(cell_limbs(elements(5, 33)[4], canonical), np.uint64)
        sel = cfg.lookup_quotient_selectors(K, EXT_K, N_ROWS, shift_limbs(nr.ZETA, canonical), canonical=canonical)
        _CHAIN[canonical] = dict(cfg=cfg, ch=ch, z=z, y=y, sel=sel, chars=np.ascontiguousarray(chars[keep]), lens=lens[keep])
    return _CHAIN[canonical]


def chain_quotient(c, canonical, tamper=None, divide=False):
    cfg, ch = c["cfg"], c["ch"]
    cols, S = lagrange_columns(cfg, ch, c["z"], seed=5, tamper=tamper)
    ext = {name: to_coset(cfg, a, canonical, nr.ZETA) for name, a in cols.items()}
    s_ext = to_coset(cfg, S, canonical, nr.ZETA)
    t = cfg.fr_vanishing_inverse_host(K, EXT_K, shift_limbs(nr.ZETA, canonical), canonical=canonical) if divide else None
    h = cfg.lookup_quotient_host(K, EXT_K, ext["A"], ext["Ap"], ext["Sp"], ext["Z"], s_ext, c["sel"], ch.beta, ch.gamma, c["y"], t_inv=t, divide=divide,
                                 canonical=canonical)
    return ext, s_ext, h


def folded(coeffs, n, rows):
    """sum_c coeff[i + c n] for i in rows: the polynomial modulo X^n - 1"""
    return [sum(coeffs[i + c * n] for c in range(len(coeffs) // n)) % R for i in rows]


@pytest.mark.parametrize("canonical", [False, True])
def test_the_chain_on_the_host(canonical):
    c = host_chain(canonical)
    cfg, ch = c["cfg"], c["ch"]
    n, N, B = 1 << K, 1 << EXT_K, ch.B
    ext, s_ext, h = chain_quotient(c, canonical)
    sel = tuple(nr.values_of(c["sel"][i], canonical) for i in range(3))
    beta, gamma, y = (nr.values_of(x, canonical)[0] for x in (ch.beta, ch.gamma, c["y"]))
    zeta_inv = shift_limbs(pow(nr.ZETA, -1, R), canonical)
    _, _, q = chain_quotient(c, canonical, divide=True)
    h_coeff = cfg.fr_ntt_host(h, EXT_K, inverse=True, shift=zeta_inv, canonical=canonical)
    q_coeff = cfg.fr_ntt_host(q, EXT_K, inverse=True, shift=zeta_inv, canonical=canonical)
    for b in range(B):
        lookups = [{name: nr.values_of(ext[name][col, b], canonical) for name in ("A", "Ap", "Sp", "Z")} for col in range(3)]
        for col in range(3):
            lookups[col]["S"] = nr.values_of(s_ext[col], canonical)
        assert np.array_equal(h[b], nr.cells_of(qr.fold(K, EXT_K, lookups, sel, beta, gamma, y), canonical)), b      # every point
        hc, qc = nr.values_of(h_coeff[b], canonical), nr.values_of(q_coeff[b], canonical)
        assert any(hc) and folded(hc, n, range(n)) == [0] * n, "h vanishes on the rows: zero modulo X^n - 1"
        assert not any(qc[3 * n:]), "the quotient has degree below 3 n"
        assert all(hc[i] == ((qc[i - n] if i >= n else 0) - qc[i]) % R for i in range(N)), "h = (X^n - 1) q"


def test_a_tampered_z_entry_breaks_the_fold():
    c = host_chain(False)
    cfg, n = c["cfg"], 1 << K
    zeta_inv = shift_limbs(pow(nr.ZETA, -1, R), False)
    for tamper in [(0, 0, 1), (1, 1, 2000), (2, 2, N_ROWS)]:
        _, _, h = chain_quotient(c, False, tamper=tamper)
        coeff = cfg.fr_ntt_host(h, EXT_K, inverse=True, shift=zeta_inv)
        for b in range(3):
            zero = folded(nr.values_of(coeff[b], False), n, range(n)) == [0] * n
            assert zero == (b != tamper[1]), (tamper, b)


# ---- the rule under the sanitizers --------------------------------------------------------------------------------------------------------------------
def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_quotient_host.cpp: csrc/hrx_fr.h + csrc/hrx_quotient.hpp + csrc/hrx_quotient_host.cpp compiled into a program of their own with the
    address and undefined-behaviour sanitizers — the host twin at k <= 4 against the five steps over a schoolbook product, every buffer a heap block of its
    exact size"""
    exe = str(tmp_path / "hrx_test_quotient_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_quotient_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "quotient host: ok" in out.stdout, out.stdout + out.stderr
