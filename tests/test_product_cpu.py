"""LOOKUP PRODUCT on the host (include/hrx.h hrx_lookup_invert_table_host / hrx_lookup_product_host on host-only contexts; csrc/hrx_product.hpp): the inverse
tables against pow(x, -1, r), the grand product against product_ref — Python integers, the rule transcribed — limb for limb through the whole chain
counts -> compress -> permute -> invert -> product, the closing property, halo2's constraint over the returned cells, what a tampered record, a bad index and
a zero denominator do, the layout and the contract, and the rule as a program of its own under the sanitizers.  No device."""
import os
import subprocess

import numpy as np
import pytest

import halo2_regex_amd as hra
import product_ref as pr
from compress_ref import R, cell_limbs, int_of, limbs_of
from oracle_lib import ROOT
from test_lookup_cpu import small_batch
from test_match_cpu import CFG_1, CFG_23, CFG_H4, _cfg
from test_permute_cpu import lookups_of, t_max

SETS = {"regex1": CFG_1, "regex23": CFG_23, "five": CFG_H4 + CFG_23[:1]}
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
NO_ROW = 0xffffffff
M = 64


def challenges(count, seed, canonical):
    """(count, 4) uint64 limbs of seeded elements in the call's limb form"""
    rng = np.random.default_rng(seed)
    return np.array([cell_limbs(int.from_bytes(rng.bytes(32), "little") % R, canonical) for _ in range(count)], np.uint64)


def batch(cfg):
    """small_batch's strings (n = 0, 1, M - 1, M — the row M - 1 rule — and ragged noise) and one whose length is set to M + 1 behind the walk: no rows"""
    chars, lens = small_batch(M)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    lens = lens.copy()
    lens[-1] = M + 1
    return chars, lens, rec


class Chain:
    """the host chain of one window: counts, compressed inputs and table, the permuted index columns, the two inverse tables"""

    def __init__(self, cfg, chars, lens, rec, n_rows, canonical=False, per_string=False, seed=1):
        B = len(lens)
        self.cfg, self.lens, self.n_rows, self.canonical, self.B, self.M = cfg, lens, n_rows, canonical, B, cfg.max_chars_size
        self.counts, self.misses = cfg.lookup_counts_host(chars, lens, rec)
        ch = challenges(3 * B, seed, canonical).reshape(3, B, 4)
        self.theta, self.beta, self.gamma = (ch[i] if per_string else ch[i, 0] for i in range(3))
        self.table = cfg.lookup_compress_table_host(self.theta, canonical=canonical)
        if not per_string:
            self.table = self.table[0]
        self.inputs = cfg.lookup_compress_inputs_host(chars, lens, rec, self.theta, canonical=canonical)
        perm = cfg.lookup_permute_host(self.counts, n_rows, out=("idx",))
        self.a_idx, self.s_idx, self.overflow = perm["a_idx"], perm["s_idx"], perm["overflow"]
        self.inv_beta = cfg.lookup_invert_table_host(self.table, self.beta, canonical=canonical)
        self.inv_gamma = cfg.lookup_invert_table_host(self.table, self.gamma, canonical=canonical)

    def product(self, a_idx=None, s_idx=None, inv_beta=None, beta=None, **kw):
        return self.cfg.lookup_product_host(self.lens, self.inputs, self.a_idx if a_idx is None else a_idx, self.s_idx if s_idx is None else s_idx, self.n_rows,
                                            self.table, self.inv_beta if inv_beta is None else inv_beta, self.inv_gamma, self.beta if beta is None else beta,
                                            self.gamma, canonical=self.canonical, **kw)

    def ref(self, a_idx=None, s_idx=None, beta=None, strings=None):
        return pr.product(lookups_of(self.cfg), self.lens, self.M, self.inputs, self.a_idx if a_idx is None else a_idx, self.s_idx if s_idx is None else s_idx,
                          self.n_rows, self.table, self.beta if beta is None else beta, self.gamma, self.canonical, strings=strings)

    def honest(self):
        """the strings whose every input is in its table (or which have no rows) and whose lookups fit the circuit"""
        return [b for b in range(self.B) if (self.misses[b] == 0 or int(self.lens[b]) > self.M) and self.overflow[b] == 0]


# ---- the inverse tables -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("name", ["regex1", "regex23"])
def test_invert_against_python_integers(name, canonical):
    cfg = _cfg(SETS[name], M)
    W, bins = cfg.lookup_words(), max(sl.stop for _, sl in lookups_of(cfg))
    theta = challenges(1, 5, canonical)[0]
    table = cfg.lookup_compress_table_host(theta, canonical=canonical)[0]
    S = pr.values_of(table, canonical)
    chosen = [0, bins // 2, bins - 1]
    shifts = [0, 1, R - 1] + [(-S[w]) % R for w in chosen]
    # every shift as limbs of a run of its own (shift_stride 4), and the first as one for the call (0); a shift of c + r means c
    limbs = np.array([cell_limbs(c, canonical) for c in shifts], np.uint64)
    inv = cfg.lookup_invert_table_host(np.broadcast_to(table, (len(shifts), W, 4)), limbs, canonical=canonical)
    for t, c in enumerate(shifts):
        vals = pr.values_of(inv[t], canonical)
        zeros = [w for w in range(bins) if (S[w] + c) % R == 0]
        assert set(chosen[t - 3:t - 2] if t >= 3 else []) <= set(zeros)
        for w in range(bins):
            assert vals[w] * (S[w] + c) % R == (0 if w in zeros else 1), (t, w)
            assert w not in zeros or vals[w] == 0
        assert not inv[t, bins:].any(), "pad words are zero cells"
        assert np.array_equal(inv[t], pr.inverse_table(table, bins, limbs[t], canonical))
    one = cfg.lookup_invert_table_host(table, limbs[1], canonical=canonical)
    assert one.shape == (W, 4) and np.array_equal(one, inv[1])
    unreduced = np.array(limbs_of(int_of(limbs[1]) + R), np.uint64)           # taken mod r first
    assert np.array_equal(cfg.lookup_invert_table_host(table, unreduced, canonical=canonical), inv[1])


# ---- the host twin against the yardstick, and what the columns must satisfy ---------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("name", list(SETS))
def test_host_twin_against_product_ref(name, canonical):
    cfg = _cfg(SETS[name], M)
    chars, lens, rec = batch(cfg)
    assert {0, M, M + 1} <= set(int(n) for n in lens)
    for n_rows in (t_max(cfg) + 1, 4090):
        ch = Chain(cfg, chars, lens, rec, n_rows, canonical, per_string=n_rows != 4090, seed=n_rows)
        res = ch.product()
        assert res["z"].shape == (3 * cfg.num_defs, ch.B, (n_rows + 4) & ~3, 4)
        honest = ch.honest()
        assert {0, M, M + 1} <= set(int(lens[b]) for b in honest)
        # the yardstick on every string (five defs at 4090 rows: on the edge lengths and two more)
        sample = range(ch.B) if name != "five" or n_rows != 4090 else sorted({b for b in range(ch.B) if int(lens[b]) in (0, M, M + 1)} | {ch.B - 2, ch.B - 3})
        z, opened, ints = ch.ref(strings=sample)
        for b in sample:
            assert np.array_equal(res["z"][:, b, :n_rows + 1], z[:, b]), (b, n_rows)
            assert res["open"][b] == opened[b]
            assert not res["z"][:, b, n_rows + 1:].any()
        # the closing property
        one = np.array(cell_limbs(1, canonical), np.uint64)
        for b in honest:
            assert res["open"][b] == 0 and (res["z"][:, b, n_rows] == one).all() and (res["z"][:, b, 0] == one).all(), b
        for b in set(range(ch.B)) - set(honest):
            assert res["open"][b] != 0, b


@pytest.mark.parametrize("canonical", [False, True])
def test_constraint_of_the_lookup_argument_over_the_returned_cells(canonical):
    cfg = _cfg(CFG_23, M)
    chars, lens, rec = batch(cfg)
    n_rows = t_max(cfg) + 1
    ch = Chain(cfg, chars, lens, rec, n_rows, canonical, per_string=True, seed=3)
    res = ch.product()
    for b in range(ch.B):
        S = pr.values_of(ch.table[b], canonical)
        beta, gamma = pr.challenge_value(ch.beta[b], canonical), pr.challenge_value(ch.gamma[b], canonical)
        for col, sl in lookups_of(cfg):
            Z = pr.values_of(res["z"][col, b, :n_rows + 1], canonical)
            A_in = pr.values_of(ch.inputs[col, b], canonical)
            off, T, n = sl.start, sl.stop - sl.start, int(lens[b])
            assert Z[0] == 1
            for i in range(n_rows):
                A = S[off] if i >= M or n > M or (n == M and i == M - 1 and col % 3 != 1) else A_in[i]
                Si = S[off + i] if i < T else S[off]
                Ap, Sp = S[ch.a_idx[col, b, i]], S[ch.s_idx[col, b, i]]
                assert Z[i + 1] * (Ap + beta) * (Sp + gamma) % R == Z[i] * (A + beta) * (Si + gamma) % R, (b, col, i)


# ---- what goes wrong must end in `open` ---------------------------------------------------------------------------------------------------------
def test_a_tampered_record_opens_its_lookup_and_no_other_string():
    cfg = _cfg(CFG_23, M)
    chars, lens, rec = batch(cfg)
    n_rows = t_max(cfg) + 1
    clean = Chain(cfg, chars, lens, rec, n_rows)
    b = next(b for b in clean.honest() if int(lens[b]) == M - 1)
    rec = rec.copy()
    rec[b, 3, 1] = (rec[b, 3, 1] & ~np.uint32(0xffff)) | np.uint32(0xfff0)          # def 1, row 3: a state outside every table
    ch = Chain(cfg, chars, lens, rec, n_rows)
    assert ch.misses[b] != 0 and (np.delete(ch.misses, b) == np.delete(clean.misses, b)).all()
    z, opened, ints = ch.ref()
    bits = int(opened[b])
    assert bits & (1 << 3) and not bits & 0b111, "the yardstick alone, for these challenges: def 1's transition lookup opens, def 0's lookups close"
    assert all(opened[x] == 0 for x in clean.honest() if x != b)
    res = ch.product()
    assert np.array_equal(res["open"], opened) and np.array_equal(res["z"][:, :, :n_rows + 1], z)


def test_bad_indices_and_a_zero_denominator():
    cfg = _cfg(CFG_23, M)
    chars, lens, rec = batch(cfg)
    n_rows = t_max(cfg) + 1
    ch = Chain(cfg, chars, lens, rec, n_rows)
    b, b2 = ch.honest()[:2]
    looks = lookups_of(cfg)
    zero = np.zeros(4, np.uint64)
    # permute's overflow pattern in lookup 0 of string b; an index of lookup 4's range in row 5 of lookup 1 of string b2
    a_idx, s_idx = ch.a_idx.copy(), ch.s_idx.copy()
    a_idx[0, b, :n_rows] = s_idx[0, b, :n_rows] = NO_ROW
    s_idx[1, b2, 5] = looks[4][1].start
    res = ch.product(a_idx=a_idx, s_idx=s_idx)
    z, opened, ints = ch.ref(a_idx=a_idx, s_idx=s_idx)
    assert np.array_equal(res["z"][:, :, :n_rows + 1], z) and np.array_equal(res["open"], opened)
    assert res["open"][b] == 1 and res["open"][b2] == 2, "the bit is set and the string's other lookups close"
    assert (res["z"][0, b, 1:n_rows + 1] == zero).all() and res["z"][0, b, 0].any(), "zero from row 1"
    assert res["z"][1, b2, 5].any() and (res["z"][1, b2, 6:n_rows + 1] == zero).all()
    assert [int(res["open"][x]) for x in ch.honest() if x not in (b, b2)] == [0] * (len(ch.honest()) - 2), "the other strings and lookups close"
    # a zero denominator: beta = -S'[j] of lookup 0 of string b — Z is zero from j + 1 (and wherever another lookup of the call meets that cell)
    j = 7
    S = pr.values_of(ch.table, False)
    beta = np.array(cell_limbs((-S[ch.a_idx[0, b, j]]) % R, False), np.uint64)
    inv_beta = cfg.lookup_invert_table_host(ch.table, beta)
    assert not inv_beta[ch.a_idx[0, b, j]].any()
    res = ch.product(beta=beta, inv_beta=inv_beta)
    z, opened, ints = ch.ref(beta=beta)
    assert np.array_equal(res["z"][:, :, :n_rows + 1], z) and np.array_equal(res["open"], opened)
    first = int(np.nonzero(ch.a_idx[0, b, :n_rows] == ch.a_idx[0, b, j])[0][0])
    assert res["z"][0, b, first].any() and (res["z"][0, b, first + 1:n_rows + 1] == zero).all() and first <= j and res["open"][b] & 1


# ---- layout and contract ------------------------------------------------------------------------------------------------------------------------
def test_z_between_guards_and_refused_calls_write_nothing():
    cfg = _cfg(CFG_23, 5)
    W, ncols, T = cfg.lookup_words(), 3 * cfg.num_defs, t_max(cfg)
    B, n_rows, Mc = 2, T + 2, 5
    ip, zp = (n_rows + 3) & ~3, (n_rows + 4) & ~3
    lens = np.array([3, 5], np.uint32)
    inputs = np.zeros((ncols, B, Mc, 4), np.uint64)
    idx = np.zeros((ncols, B, ip), np.uint32)
    table, ib, ig = (np.zeros((W, 4), np.uint64) for _ in range(3))
    bg = np.zeros((2, 4), np.uint64)
    z = np.full(ncols * B * zp * 4 + 2, POISON64, np.uint64)         # 16 bytes of slack: a pointer 8 bytes further is misaligned and still inside
    op = np.full(B + 1, POISON32, np.uint32)
    f, g, ctx = hra.lib.hrx_lookup_product_host, hra.lib.hrx_lookup_product_device, cfg._ctx
    P = lambda a, off=0: a.ctypes.data + off
    good = dict(lens=P(lens), M=Mc, b_begin=0, b_count=B, in_cells=P(inputs), a_idx=P(idx), s_idx=P(idx), n_rows=n_rows, idx_pitch=ip, table=P(table), ib=P(ib),
                ig=P(ig), tstride=0, beta=P(bg), gamma=P(bg, 32), cstride=0, z=P(z), z_pitch=zp, open=P(op), flags=0)
    order = list(good)

    def call(fn=f, tail=(), **kw):
        a = dict(good, **kw)
        return fn(ctx, *[a[k] for k in order], *tail)

    bad = [dict(n_rows=T - 1), dict(n_rows=(1 << 24) + 1, idx_pitch=0, z_pitch=0), dict(idx_pitch=ip - 4), dict(idx_pitch=ip + 2), dict(z_pitch=n_rows),
           dict(z_pitch=zp + 2), dict(tstride=4), dict(tstride=4 * W + 4), dict(cstride=8), dict(flags=2), dict(flags=-1)]
    bad += [{k: None} for k in ("lens", "in_cells", "a_idx", "s_idx", "table", "ib", "ig", "beta", "gamma", "z")]
    bad += [dict(in_cells=P(inputs, 8)), dict(a_idx=P(idx, 4)), dict(s_idx=P(idx, 8)), dict(table=P(table, 8)), dict(ib=P(ib, 8)), dict(ig=P(ig, 8)),
            dict(z=P(z, 8)), dict(open=P(op, 2)), dict(beta=P(bg, 4))]
    for kw in bad:
        assert call(**kw) == hra.HRX_ERR_ARG, kw
        assert (z == POISON64).all() and (op == POISON32).all(), kw
    assert f(None, *[good[k] for k in order]) == hra.HRX_ERR_ARG
    assert call(b_count=0) == hra.HRX_OK and (z == POISON64).all()
    assert call(g, tail=(None,)) == hra.HRX_ERR_HIP and (z == POISON64).all(), "the device form on a host-only context: the argument rules first"
    assert call(g, tail=(None,), z_pitch=n_rows) == hra.HRX_ERR_ARG
    assert call(z_pitch=0) == hra.HRX_OK and call(idx_pitch=0) == hra.HRX_OK and call(open=None) == hra.HRX_OK
    zz = z[:ncols * B * zp * 4].reshape(ncols, B, zp, 4)
    assert (zz[:, :, :n_rows + 1] != POISON64).all() and (zz[:, :, n_rows + 1:] == POISON64).all() and (z[-2:] == POISON64).all(), "entries above n_rows are the caller's"
    assert op[B] == POISON32 and (op[:B] != POISON32).all()
    # a wider pitch, the poison kept; the invert call's refusals
    big = np.full((ncols, B, 1 << n_rows.bit_length(), 4), POISON64, np.uint64)
    res = cfg.lookup_product_host(lens, inputs, idx, idx, n_rows, table, ib, ig, bg[0], bg[1], z_pitch=big.shape[2], out={"z": big})
    assert res["z"] is big and (big[:, :, n_rows + 1:] == POISON64).all() and (big[:, :, :n_rows + 1] != POISON64).all()
    inv = np.full(W * 4 + 2, POISON64, np.uint64)
    fi, gi = hra.lib.hrx_lookup_invert_table_host, hra.lib.hrx_lookup_invert_table_device
    for args in [(None, 1, P(bg), 0, P(inv), 0), (P(table), 1, None, 0, P(inv), 0), (P(table), 1, P(bg), 0, None, 0), (P(table, 8), 1, P(bg), 0, P(inv), 0),
                 (P(table), 1, P(bg), 0, P(inv, 8), 0), (P(table), 1, P(bg), 8, P(inv), 0), (P(table), 1, P(bg), 0, P(inv), 2), (P(table), 1, P(bg, 4), 0, P(inv), 0)]:
        assert fi(ctx, *args) == hra.HRX_ERR_ARG and (inv == POISON64).all(), args
    assert gi(ctx, P(table), 1, P(bg), 0, P(inv), 0, None, 0, None) == hra.HRX_ERR_HIP and (inv == POISON64).all()
    assert gi(ctx, P(table), 1, P(bg), 0, P(inv), 0, 64, 4096, None) == hra.HRX_ERR_ARG, "a misaligned workspace"
    assert fi(ctx, P(table), 1, P(bg), 0, P(inv), 0) == hra.HRX_OK and (inv[:W * 4] == 0).all() and (inv[W * 4:] == POISON64).all()
    assert cfg.lookup_invert_workspace_bytes(4096) == 0
    plan = cfg.lookup_product_plan(B, n_rows)
    assert plan["tile_rows"] % plan["rows_per_lane"] == 0 and plan["rows_per_lane"] >= 1


# ---- the rule under the sanitizers --------------------------------------------------------------------------------------------------------------
def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_cpp/test_product_host.cpp: csrc/hrx_product.hpp + csrc/hrx_product_host.cpp compiled into a program of their own with the address and
    undefined-behaviour sanitizers — the rule with a schoolbook product and an inversion by extended Euclid as the independent arithmetic, every buffer a
    heap block of its exact size"""
    exe = str(tmp_path / "hrx_test_product_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_product_host.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "product host: ok" in out.stdout, out.stdout + out.stderr
