"""LOOKUP PRODUCT on the host at edge operands and borders (hrx_lookup_invert_table_host / hrx_lookup_product_host; csrc/hrx_product.hpp, csrc/hrx_fr.h): the
host twin against Python integers on every case of product_edges.py, in both limb forms — fr_inv handed each operand of fr_edges.E alone, zero words on the
lane, wave and tile borders of runs that end on, before and behind a tile, shifts and challenges around every border of fr_reduce, a product whose every
factor is an edge operand, and M on and around a tile border.  test_product_edges_gpu.py runs the same cases through the kernels.  No device."""
import numpy as np
import pytest

import product_edges as pe
import product_ref as pr
from compress_ref import R
from fr_edges import E, POISON64, limbs_array
from test_permute_cpu import lookups_of

FORMS = [False, True]


def test_sized_sets_cover_the_run_sizes_and_pad_counts():
    """a change to synth.random_dfa or to the run layout must not quietly empty the matrix"""
    got = {}
    for bins in pe.SIZED:
        cfg = pe.sized_cfg(bins, 40)                                     # asserts bins, W and T_max itself
        got[pe.run_bins(cfg)] = cfg.lookup_words() - pe.run_bins(cfg)
    assert sorted(got) == [39, 42, 1023, 1024, 1025, 2047, 2048, 2049, 2057]
    assert set(got.values()) == {0, 1, 2, 3} and got[42] == 2 and got[1024] == got[2048] == 0 and got[1025] == got[2049] == 3
    tile = 1024
    assert {b - tile * (b // tile) for b in got if b > 1000} >= {0, 1, tile - 1}, "a run one word short of a tile, on it, one word into the next"
    assert pe.BORDERS(2057) == [0, 1, 3, 4, 5, 255, 256, 1023, 1024, 1025, 1028, 2047, 2048, 2055, 2056] and pe.BORDERS(39) == [0, 1, 3, 4, 5, 19, 37, 38]
    assert len(pe.WIDE_SHIFTS) == 9 and all(v >= R for v in pe.WIDE_SHIFTS[:8])


# ---- the inverse tables -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("bins,positions,c", [(2057, None, int.from_bytes(np.random.default_rng(8).bytes(32), "little") % R), (39, (0, 3, 4, 38), pe.WIDE_SHIFTS[6])],
                         ids=["2057-bins", "39-bins"])
def test_fr_inv_is_handed_every_edge_operand_alone(bins, positions, c, canonical):
    cfg = pe.sized_cfg(bins, 40)
    W = cfg.lookup_words()
    table, cases = pe.isolation_runs(bins, W, E, pe.BORDERS(bins) if positions is None else positions, c)
    assert len(cases) == len(E) * (15 if positions is None else 4)
    got = cfg.lookup_invert_table_host(table, limbs_array([c])[0], canonical=canonical)
    pe.check(pe.first_wrong_isolation(got, cases, W, canonical))
    # the expectation against the yardstick, on the runs of one position
    for t in range(0, len(cases), len(cases) // len(E)):
        assert np.array_equal(pe.isolation_expected(cases, W, canonical)[t], pr.inverse_table(table[t], bins, limbs_array([c])[0], canonical)), cases[t]


@pytest.mark.parametrize("canonical", FORMS)
def test_a_run_of_zero_words_only(canonical):
    """the total is one and every output the zero cell"""
    for bins in (39, 2057):
        cfg = pe.sized_cfg(bins, 40)
        table, cases = pe.isolation_runs(bins, cfg.lookup_words(), [0], [0], pe.WIDE_SHIFTS[-1])
        got = cfg.lookup_invert_table_host(table[0], limbs_array([pe.WIDE_SHIFTS[-1]])[0], canonical=canonical)
        assert got.shape == (cfg.lookup_words(), 4) and not got.any()


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("bins", list(pe.SIZED))
def test_zero_words_on_every_border_of_every_run_size(bins, canonical):
    cfg = pe.sized_cfg(bins, 40)
    for group in range(pe.ZERO_GROUPS):
        table, shifts, want, planted = pe.zero_pattern_case(bins, canonical, group)
        assert shifts.shape == ((4,) if group == 3 else (3, 4))
        assert (table[:, bins:] == POISON64).all() and set(pe.BORDERS(bins)) < set(planted)
        got = cfg.lookup_invert_table_host(table, shifts, canonical=canonical)
        pe.check(pe.first_wrong_word(got, want, shifts, canonical))
        assert not got[:, bins:].any() and not got[:, planted].any(), "pad words and zero words are zero cells"
        assert np.array_equal(cfg.lookup_invert_table_host(table, pe.reduced(shifts), canonical=canonical), got), "a shift means its value mod r"


# ---- the product --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
def test_a_product_whose_every_factor_is_an_edge_operand(canonical):
    cfg = pe.sized_cfg(39, 40)
    m = pe.operand_matrix(cfg, canonical)
    assert lookups_of(cfg) == m["looks"]
    call = lambda **kw: cfg.lookup_product_host(m["lens"], m["inputs"], m["a_idx"], m["s_idx"], m["n_rows"], m["table"], m["inv_beta"], m["inv_gamma"], m["beta"],
                                                m["gamma"], canonical=canonical, **kw)
    res = call()
    pe.check(pe.first_wrong_z(res["z"], m["z"], m["n_rows"], canonical))
    assert np.array_equal(res["open"], m["open"]) and (m["open"] & 1).all()
    closed = call(open=False)
    assert set(closed) == {"z"} and np.array_equal(closed["z"], res["z"])
    again = cfg.lookup_product_host(m["lens"], m["inputs"], m["a_idx"], m["s_idx"], m["n_rows"], m["table"], m["inv_beta"], m["inv_gamma"], pe.reduced(m["beta"]),
                                    pe.reduced(m["gamma"]), canonical=canonical)
    assert np.array_equal(again["z"], res["z"]) and np.array_equal(again["open"], res["open"])


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("bins,M,n_rows", pe.m_border_cases())
def test_M_on_and_around_a_tile_border(bins, M, n_rows, canonical):
    ch, z, opened = pe.m_border_chain(bins, M, n_rows, canonical)
    assert [int(n) for n in ch.lens] == [M, M - 1, 0, 1] and ch.M == M
    res = ch.product()
    what = "M %d: " % M
    pe.check(pe.first_wrong_z(res["z"], z, n_rows, canonical, what))
    assert np.array_equal(res["open"], opened) and not res["z"][:, :, n_rows + 1:].any()
    # the counts cover all M rows of every string: with n_rows >= M everything fits and closes, with n_rows < M - 1 every lookup overflows and opens
    honest = ch.honest()
    assert not ch.misses.any() and not opened[honest].any() and all(opened[b] for b in range(ch.B) if b not in honest)
    assert len(honest) == ch.B if n_rows >= M else n_rows >= M - 1 or (ch.overflow == 7).all() and (opened == 7).all()


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("per_string", [False, True])
def test_wide_challenges_into_the_product(per_string, canonical):
    ch = pe.wide_challenge_chain(canonical, per_string)
    cfg = ch.cfg
    for beta, gamma in pe.wide_challenge_pairs(per_string):
        ib, ig = (cfg.lookup_invert_table_host(ch.table, c, canonical=canonical) for c in (beta, gamma))
        assert np.array_equal(ib, cfg.lookup_invert_table_host(ch.table, pe.reduced(beta), canonical=canonical))
        res = cfg.lookup_product_host(ch.lens, ch.inputs, ch.a_idx, ch.s_idx, ch.n_rows, ch.table, ib, ig, beta, gamma, canonical=canonical)
        low = cfg.lookup_product_host(ch.lens, ch.inputs, ch.a_idx, ch.s_idx, ch.n_rows, ch.table, ib, ig, pe.reduced(beta), pe.reduced(gamma), canonical=canonical)
        assert np.array_equal(res["z"], low["z"]) and np.array_equal(res["open"], low["open"]), "a challenge means its value mod r"
        z, opened, ints = pr.product(lookups_of(cfg), ch.lens, ch.M, ch.inputs, ch.a_idx, ch.s_idx, ch.n_rows, ch.table, beta, gamma, canonical)
        what = "beta %#x: " % pe.int_of(beta.reshape(-1, 4)[0])
        pe.check(pe.first_wrong_z(res["z"], z, ch.n_rows, canonical, what))
        assert np.array_equal(res["open"], opened)
