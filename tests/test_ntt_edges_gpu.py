"""The field arithmetic under FR NTT on edge operands, on the device (csrc/hrx_fr.h as the device compiler builds it into carry chains, through
hrx_fr_ntt_device): what test_ntt_edges_cpu.py puts through the host twin, through the kernel — every buffer between poisoned guards, every call against the
host twin limb for limb and then against Python integers:
  size 2               every ordered pair of fr_edges.E as a column of one k = 1 call (1089 columns, 512 to a workgroup): fr_add and fr_sub, with a shift one
                       fr_mul more; both directions and limb forms; the shifts none, 0, r, r + 1, 2^256 - 1 and a quarter of E per direction and form
  size 4               every ordered 4-tuple of six of the values against the naive sums
  whole tiles          k = 12 (the whole-LDS tile), 13 (the first permuting size) and a packed k: columns of edge values, columns whose stage-0 sums are all
                       exactly r and columns whose stage-0 differences are all 0
Every input cell is below r; only the shift is handed over unreduced."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fr_edges as fe
from test_ntt_edges_cpu import PAIRS, TUPLE_CALLS, TUPLE_IDS
from test_ntt_gpu import G, PACKED, plan, same_as_host, workspaces_unchanged
from test_ntt_gpu import release_the_shared_context  # noqa: F401  (the workspaces and the context this module takes from test_ntt_gpu go with it as well)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_every_pair_of_edge_operands_through_size_2(inverse, canonical):
    cells = fe.tuple_cells(PAIRS)
    assert plan(1)["cols_per_group"] < len(PAIRS), "more than one workgroup"
    quarter = fe.E[2 * inverse + canonical::4]                                               # the four tests together: every value of E as a shift
    for s in dict.fromkeys([None, 0] + fe.UNREDUCED + quarter):
        got = same_as_host(1, len(PAIRS), n_in=2, inverse=inverse, canonical=canonical, cells=cells, shift=fe.shift_limbs(s))
        wrong = fe.first_wrong_pair(got, PAIRS, s, inverse, canonical)
        assert wrong is None, wrong
    got = same_as_host(1, len(PAIRS), n_in=2, inverse=inverse, canonical=canonical, cells=cells, shift=fe.shift_limbs(fe.ALL_ONES), in_place=True)
    assert fe.first_wrong_pair(got, PAIRS, fe.ALL_ONES, inverse, canonical) is None
    assert workspaces_unchanged()


@pytest.mark.parametrize("inverse,canonical,g", TUPLE_CALLS, ids=TUPLE_IDS)
def test_every_4_tuple_of_six_edge_operands_against_the_naive_sums(inverse, canonical, g):
    tuples = list(itertools.product(fe.SIX, repeat=4))
    got = same_as_host(2, len(tuples), inverse=inverse, canonical=canonical, g=g, cells=fe.tuple_cells(tuples))
    assert np.array_equal(got, fe.naive_of_tuples(tuples, 2, inverse, canonical, g))


@pytest.mark.parametrize("k", [PACKED, 12, 13])
def test_edge_values_in_whole_tiles(k):
    n, cells = 1 << k, fe.tile_columns(k, k)
    fwd = same_as_host(k, 3, cells=cells)
    assert not fwd[1, 0::2].any(), "x[i + n/2] = r - x[i]: every stage-0 sum is r, every even output the zero cell"
    assert not fwd[2, 1::2].any(), "x[i + n/2] = x[i]: every stage-0 difference is 0, every odd output the zero cell"
    same_as_host(k, 3, canonical=True, g=G, cells=cells, out_pitch=n + 4)
    same_as_host(k, 3, inverse=True, cells=cells)
    same_as_host(k, 3, inverse=True, cells=cells, shift=fe.shift_limbs(fe.ALL_ONES), in_place=True)
    assert workspaces_unchanged()
