"""The field arithmetic under FR NTT on edge operands, on the host (csrc/hrx_fr.h as the host compiler builds it, through hrx_fr_ntt_host): every ordered pair of
fr_edges.E as a column of one k = 1 call — a transform of size 2 is fr_add and fr_sub, and with a shift one fr_mul more — against Python integers, limb for
limb: both directions, both limb forms, the shifts none, every value of E, and r, r + 1, 2^256 - 1 (taken mod r first; g = 0 gives g^0 = 1 and g^1 = 0).  Then
every ordered 4-tuple of six of the values at k = 2 against the naive sums, and edge values in whole columns.  No device."""
import itertools

import numpy as np
import pytest

import fr_edges as fe
import ntt_ref as nr
from compress_ref import R, cell_limbs, int_of
from test_ntt_cpu import cfg

PAIRS = fe.pairs()


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_every_pair_of_edge_operands_through_size_2(inverse, canonical):
    cells = fe.tuple_cells(PAIRS)
    keep = cells.copy()
    for s in [None] + fe.E + fe.UNREDUCED:
        out = np.full_like(cells, fe.POISON64)
        cfg().fr_ntt_host(cells, 1, out=out, inverse=inverse, n_in=2, shift=fe.shift_limbs(s), canonical=canonical)
        wrong = fe.first_wrong_pair(out, PAIRS, s, inverse, canonical)
        assert wrong is None, wrong
        assert (out[:, 2:] == fe.POISON64).all() and np.array_equal(cells, keep)
    in_place = cells.copy()
    assert cfg().fr_ntt_host(in_place, 1, out=in_place, inverse=inverse, n_in=2, shift=fe.shift_limbs(fe.ALL_ONES), canonical=canonical) is in_place
    assert fe.first_wrong_pair(in_place, PAIRS, fe.ALL_ONES, inverse, canonical) is None and (in_place[:, 2:] == fe.POISON64).all()


def test_the_expectation_is_the_two_sums():
    """size_2, the stored-value formulas the pair matrix is held against, is ntt_ref.naive at k = 1 on the values the cells stand for"""
    for canonical in (False, True):
        for inverse in (False, True):
            for a, b, g in [(5, 9, 7), (R - 1, 1, R - 1), (fe.ALL_ONES, fe.E[11], 3), (0, 2, 0)]:
                stored = fe.size_2(a, b, int_of(cell_limbs(g, canonical)), inverse, canonical)
                want = nr.naive(nr.values_of(fe.limbs_array([a, b]), canonical), 1, inverse, g)
                assert nr.values_of(fe.limbs_array(stored), canonical) == want, (a, b, g, inverse, canonical)


TUPLE_CALLS = [(False, False, None), (False, True, nr.ZETA), (True, False, 7), (True, True, None)]          # (inverse, canonical, g)
TUPLE_IDS = ["forward", "forward-canonical-zeta", "inverse-7", "inverse-canonical"]


@pytest.mark.parametrize("inverse,canonical,g", TUPLE_CALLS, ids=TUPLE_IDS)
def test_every_4_tuple_of_six_edge_operands_against_the_naive_sums(inverse, canonical, g):
    tuples = list(itertools.product(fe.SIX, repeat=4))
    out = cfg().fr_ntt_host(fe.tuple_cells(tuples), 2, inverse=inverse, shift=None if g is None else nr.cells_of([g], canonical)[0], canonical=canonical)
    assert np.array_equal(out, fe.naive_of_tuples(tuples, 2, inverse, canonical, g))


@pytest.mark.parametrize("k", [5, 12])
def test_columns_whose_first_stage_sums_are_r_and_whose_differences_are_zero(k):
    cells = fe.tile_columns(k, k)
    n = 1 << k
    assert all(int_of(c) < R for c in cells.reshape(-1, 4)[::97])
    fwd = cfg().fr_ntt_host(cells, k)
    assert not fwd[1, 0::2].any(), "x[i + n/2] = r - x[i]: every even output is the zero cell"
    assert not fwd[2, 1::2].any(), "x[i + n/2] = x[i]: every odd output is the zero cell"
    assert np.array_equal(cfg().fr_ntt_host(fwd, k, inverse=True), cells)
    if k == 5:
        for c in range(3):
            assert np.array_equal(fwd[c], nr.cells_of(nr.naive(nr.values_of(cells[c], True), k), True)), c
    assert fwd.shape == (3, n, 4)
