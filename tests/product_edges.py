"""Edge cases of LOOKUP PRODUCT (include/hrx.h hrx_lookup_invert_table_* / hrx_lookup_product_*), as builders that test_product_edges_cpu.py runs through the
host twin and test_product_edges_gpu.py through the kernels: Python integers and numpy, sharing nothing with csrc/.  Everything is in STORED-value space as
fr_edges.py describes it — a cell holds the 256-bit integer v below r whatever it stands for — so one table serves both limb forms and only the expectation
differs: the invert call answers the stored s = S + c with s^-1 R^2 in Montgomery form and with s^-1 in canonical form, 0 with 0.

The kernels (csrc/hrx_kernel_product.hip) give 4 consecutive words to a lane, 256 to a wave and 1024 to a tile, and the invert kernel's second pass walks a
tile mirrored over the lanes: BORDERS are the words on and beside those cuts, SIZED the def sets whose runs end on, one short of and one behind a tile."""
import functools

import numpy as np

import halo2_regex_amd as hra
import product_ref as pr
from halo2_regex_amd import synth
from compress_ref import R, MONT, MONT_INV, int_of
from fr_edges import E, POISON64, limbs_array
from test_permute_cpu import lookups_of, t_max

# bins of the run: (states, letters, substring pairs) of synth.random_dfa(seed=2), and the W and T_max they must give
SIZED = {39: (4, 8, 1), 42: (3, 11, 3), 1023: (8, 127, 1), 1024: (9, 113, 1), 1025: (8, 127, 3), 2047: (8, 255, 1), 2048: (13, 157, 1), 2049: (8, 255, 3),
         2057: (64, 32, 3)}
SIZED_W_T = {39: (40, 33), 42: (44, 34), 1023: (1024, 1017), 1024: (1024, 1018), 1025: (1028, 1017), 2047: (2048, 2041), 2048: (2048, 2042),
             2049: (2052, 2041), 2057: (2060, 2049)}
# 256-bit values around every border of fr_reduce (4r, 2r, r): shifts, beta and gamma only, never cells
WIDE_SHIFTS = [R, R + 1, 2 * R - 1, 2 * R, 4 * R - 1, 4 * R, 5 * R + 3, 2**256 - 1, int.from_bytes(np.random.default_rng(256).bytes(32), "little")]
assert all(R <= v < 2**256 for v in WIDE_SHIFTS[:-1]) and WIDE_SHIFTS[-1] < 2**256
FORMS = {False: "Montgomery", True: "canonical"}


def check(wrong):
    """fail with what a first_wrong_* function names, pass on None"""
    assert wrong is None, wrong


def run_bins(cfg):
    return max(sl.stop for _, sl in lookups_of(cfg))


def sized_cfg(bins, M, device=hra.HRX_DEVICE_NONE):
    """a context of one def whose run has exactly `bins` bins"""
    states, letters, pairs = SIZED[bins]
    a_txt, sub_txt = synth.random_dfa(states, seed=2, alphabet=np.arange(letters, dtype=np.uint8), n_substr_pairs=pairs)
    cfg = hra.RegexVerifyConfig.configure(M, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub_txt)])], device=device)
    got = (run_bins(cfg), cfg.lookup_words(), t_max(cfg))
    assert got == (bins,) + SIZED_W_T[bins], "the def set of %d bins gives (bins, W, T_max) = %s" % (bins, got)
    return cfg


def BORDERS(bins):
    """the words that matter to the kernels' cut, inside the run"""
    return sorted(w for w in {0, 1, 3, 4, 5, 255, 256, 1023, 1024, 1025, 2047, 2048, bins // 2, bins - 2, bins - 1} if 0 <= w < bins)


def stored(cells):
    return [int_of(c) for c in np.asarray(cells).reshape(-1, 4)]


def inverse_of_stored(s, canonical):
    """what the invert call answers a stored sum s with"""
    return 0 if s % R == 0 else pow(s, -1, R) * (1 if canonical else MONT * MONT) % R


# ---- the inverse tables -------------------------------------------------------------------------------------------------------------------------
def isolation_runs(bins, W, operands, positions, c):
    """one run per (x, p): every bin holds -c — a zero word — and word p alone x - c, so the run's total is x and fr_inv is handed exactly x (x R where the
    call is canonical); the pad cells are poison.  Returns (table uint64 [runs][W][4], [(x, p)])"""
    c %= R
    cases = [(x, p) for x in operands for p in positions]
    assert all(0 <= x < R and 0 <= p < bins for x, p in cases)
    run = np.full((W, 4), POISON64, np.uint64)
    run[:bins] = limbs_array([(-c) % R])[0]
    table = np.broadcast_to(run, (len(cases), W, 4)).copy()
    table[np.arange(len(cases)), [p for _, p in cases]] = limbs_array([(x - c) % R for x, _ in cases])
    return table, cases


def isolation_expected(cases, W, canonical):
    """uint64 [runs][W][4]: word p the inverse of x, every other word of the run — the pads too — the zero cell"""
    want = np.zeros((len(cases), W, 4), np.uint64)
    want[np.arange(len(cases)), [p for _, p in cases]] = limbs_array([inverse_of_stored(x, canonical) for x, _ in cases])
    return want


def first_wrong_isolation(got, cases, W, canonical):
    """None where `got` is isolation_expected, else what the first wrong run is"""
    want = isolation_expected(cases, W, canonical)
    if np.array_equal(got, want):
        return None
    t, w = (int(v) for v in np.argwhere((got != want).any(axis=2))[0])
    return "operand %#x at word %d, %s, output word %d: got %#x, want %#x" % (cases[t][0], cases[t][1], FORMS[canonical], w, int_of(got[t, w]), int_of(want[t, w]))


def zero_pattern_runs(bins, W, shifts, seed):
    """one run per shift (any 256-bit value): cells from E in a seeded order, the cell -shift at BORDERS(bins) and at five consecutive words across a lane
    border; the pad cells are poison.  Returns (table uint64 [runs][W][4], shift limbs uint64 [runs][4], the planted words)"""
    rng = np.random.default_rng(seed)
    start = min(6, bins - 5)                                  # words 6 .. 10: lanes 1 and 2 of the forward pass, and of the mirrored one
    planted = sorted(set(BORDERS(bins)) | set(range(start, start + 5)))
    table = np.full((len(shifts), W, 4), POISON64, np.uint64)
    for t, s in enumerate(shifts):
        vals = [E[i] for i in rng.integers(0, len(E), bins)]
        for w in planted:
            vals[w] = (-s) % R
        table[t, :bins] = limbs_array(vals)
    return table, limbs_array(shifts), planted


ZERO_GROUPS = 4            # the calls of zero_pattern_case: three of three runs with a shift each, one of two runs under one shift


@functools.lru_cache(maxsize=None)
def zero_pattern_case(bins, canonical, group):
    """the zero patterns of one sized set with their expectation from product_ref.inverse_table, built once for every test that needs them: groups 0 .. 2 a
    run per value of a third of WIDE_SHIFTS (shift_stride 4), group 3 two runs under one shift for the call (shift_stride 0)"""
    W = SIZED_W_T[bins][0]
    one_shift = group == 3
    table, shifts, planted = zero_pattern_runs(bins, W, [WIDE_SHIFTS[6]] * 2 if one_shift else WIDE_SHIFTS[3 * group:3 * group + 3], seed=bins + group)
    want = np.stack([pr.inverse_table(table[t], bins, shifts[t], canonical) for t in range(len(table))])
    assert not want[:, planted].any() and want[:, [w for w in range(bins) if w not in planted]].any(axis=2).mean() > 0.9, "the reference alone: zeros where planted"
    for a in (table, shifts, want):
        a.setflags(write=False)
    return table, (shifts[0] if one_shift else shifts), want, planted


def first_wrong_word(got, want, shifts, canonical):
    if np.array_equal(got, want):
        return None
    t, w = (int(v) for v in np.argwhere((got != want).any(axis=2))[0])
    return "run %d (shift %#x), word %d, %s: got %#x, want %#x" % (t, int_of(shifts[t] if shifts.ndim == 2 else shifts), w, FORMS[canonical], int_of(got[t, w]),
                                                                int_of(want[t, w]))


# ---- the product --------------------------------------------------------------------------------------------------------------------------------
def first_wrong_z(got, want, n_rows, canonical, what=""):
    """None where the Z columns agree in entries [0, n_rows], else the first wrong entry"""
    g, w = got[:, :, :n_rows + 1], want[:, :, :n_rows + 1]
    if np.array_equal(g, w):
        return None
    c, b, i = (int(v) for v in np.argwhere((g != w).any(axis=3))[0])
    return "%slookup %d, string %d, entry %d of %d, %s: got %#x, want %#x" % (what, c, b, i, n_rows, FORMS[canonical], int_of(g[c, b, i]), int_of(w[c, b, i]))


def cells_of_values(values, canonical):
    return limbs_array([v % R if canonical else v * MONT % R for v in values])


def values_of_stored(vals, canonical):
    return [v if canonical else v * MONT_INV % R for v in vals]


def operand_matrix(cfg, canonical, seed=11):
    """the matrix below for a context of the 39-bin set with M = 40, whose layout it assumes"""
    res = _operand_matrix(canonical, seed)
    assert cfg.max_chars_size == res["M"] and lookups_of(cfg) == res["looks"] and cfg.lookup_words() == len(res["table"])
    return res


@functools.lru_cache(maxsize=None)
def _operand_matrix(canonical, seed):
    """The 39-bin set (T = 33 = len(E) transition rows), M = n_rows = 40, a string per operand: string b's input cells all hold E[b] - beta, so A + beta is
    E[b] as a stored value (0 and sums that land on r among them); the run of inv_beta holds E with 0 last in every lookup and a_idx cycles through the
    lookup's words in order; s_idx is seeded and valid; inv_gamma (never 0) and the table are seeded draws from E; beta and gamma are seeded 256-bit values
    left unreduced.  The tables' pad cell is poison.  Z is product_ref.product_column over these inverse values as they are.  Returns a dict of the call's
    arrays and "z" uint64 [3][33][44][4] (entries above n_rows zero), "open" uint32 [33]."""
    bins, M, n_rows = 39, 40, 40
    W, T = SIZED_W_T[bins]
    looks = [(0, slice(0, 33)), (1, slice(33, 36)), (2, slice(36, 39))]          # asserted against the context by the tests
    assert T == len(E) == 33
    rng = np.random.default_rng(seed)
    beta, gamma = (int.from_bytes(rng.bytes(32), "little") for _ in range(2))
    B = len(E)
    nonzero = [v for v in E if v]
    inputs = np.empty((3, B, M, 4), np.uint64)
    inputs[:] = limbs_array([(x - beta) % R for x in E])[None, :, None, :]
    pick = lambda count, pool: [pool[i] for i in rng.integers(0, len(pool), count)]
    tab, ig = pick(bins, E), pick(bins, nonzero)
    ib = nonzero + [0] + pick(3, nonzero) + pick(2, nonzero) + [0]
    a_idx = np.zeros((3, B, n_rows), np.uint32)
    s_idx = np.zeros((3, B, n_rows), np.uint32)
    for col, sl in looks:
        a_idx[col] = sl.start + np.arange(n_rows) % (sl.stop - sl.start)
        s_idx[col] = rng.integers(sl.start, sl.stop, (B, n_rows))
    pad = lambda vals: np.concatenate([limbs_array(vals), np.full((W - bins, 4), POISON64, np.uint64)])
    S, IB, IG = (values_of_stored(v, canonical) for v in (tab, ib, ig))
    bv, gv = (pr.challenge_value(limbs_array([c])[0], canonical) for c in (beta, gamma))
    z = np.zeros((3, B, (n_rows + 4) & ~3, 4), np.uint64)
    opened = np.zeros(B, np.uint32)
    for b in range(B):
        A = values_of_stored([(E[b] - beta) % R] * M, canonical)
        for col, sl in looks:
            Z = pr.product_column(A, M - 1, M, col, sl.start, sl.stop - sl.start, S, IB, IG, a_idx[col, b], s_idx[col, b], n_rows, bv, gv)
            z[col, b, :n_rows + 1] = cells_of_values(Z, canonical)
            opened[b] |= np.uint32((Z[n_rows] != 1) << col)
            # the zero operand comes last: a zero early in a column would hide every later product
            assert col != 0 or (all(Z[1:T]) if E[b] else not any(Z[1:])), "the reference alone: entries 1 .. 32 of lookup 0 are non-zero"
    res = dict(M=M, n_rows=n_rows, lens=np.full(B, M - 1, np.uint32), inputs=inputs, a_idx=a_idx, s_idx=s_idx, table=pad(tab), inv_beta=pad(ib), inv_gamma=pad(ig),
               beta=limbs_array([beta])[0], gamma=limbs_array([gamma])[0], z=z, open=opened, looks=looks)
    assert int(z[0, :, 1:T].any(axis=2).sum()) == 32 * 32
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def m_border_cases():
    """(bins, M, n_rows): M on and around a tile border with n_rows below, on and above it — n_rows < M among them, where permute overflows and every
    lookup of the long strings opens, the columns defined all the same"""
    return [(1023, M, n_rows) for M in (1023, 1024, 1025) for n_rows in (SIZED_W_T[1023][1], 1023, 1024, 1025, 1030)] + [(2047, 2048, n_rows) for n_rows in (2047, 2048, 2049)]


def m_border_batch(bins, M):
    """four strings of M, M - 1, 0 and 1 characters over two letters of the alphabet (the DFA is total)"""
    chars = np.tile(np.array([1, 2, 2], np.uint8), (4, M // 3 + 1))[:, :M].copy()
    return chars, np.array([M, M - 1, 0, 1], np.uint32)


@functools.lru_cache(maxsize=None)
def m_border_chain(bins, M, n_rows, canonical):
    """test_product_cpu.Chain of one case on a host-only context, with Chain.ref() as its expectation: (chain, z, open)"""
    from test_product_cpu import Chain
    cfg = sized_cfg(bins, M)
    chars, lens = m_border_batch(bins, M)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    ch = Chain(cfg, chars, lens, rec, n_rows, canonical, seed=M + n_rows)
    z, opened, ints = ch.ref()
    return ch, z, opened


@functools.lru_cache(maxsize=None)
def wide_challenge_chain(canonical, per_string):
    """the 39-bin set, M = n_rows = 40, nine strings of ragged lengths: the chain a product call with WIDE_SHIFTS as beta and gamma starts from"""
    from test_product_cpu import Chain
    M = 40
    cfg = sized_cfg(39, M)
    rng = np.random.default_rng(39)
    chars = rng.integers(0, 8, (len(WIDE_SHIFTS), M)).astype(np.uint8)
    lens = np.array([0, 1, M - 1, M, 7, 20, 33, 39, M], np.uint32)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    return Chain(cfg, chars, lens, rec, M, canonical, per_string, seed=5)


def wide_challenge_pairs(per_string):
    """the (beta, gamma) limbs of the calls: every wide value as beta with another as gamma — one call of nine strings, or nine calls"""
    pairs = limbs_array(WIDE_SHIFTS), limbs_array(WIDE_SHIFTS[3:] + WIDE_SHIFTS[:3])
    return [pairs] if per_string else list(zip(*pairs))


def reduced(limbs):
    return limbs_array([int_of(c) % R for c in np.asarray(limbs).reshape(-1, 4)]).reshape(np.asarray(limbs).shape)
