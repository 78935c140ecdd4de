"""LOOKUP PRODUCT on the device at edge operands and borders (hrx_lookup_invert_table_device / hrx_lookup_product_device, csrc/hrx_kernel_product.hip): the cases
of product_edges.py — which test_product_edges_cpu.py holds the host twin to — through the kernels, every output between poisoned guards and compared limb
for limb with the Python expectation AND with the host twin.

  fr_inv               each operand of fr_edges.E alone in a run, at every word of BORDERS: the device's Fermat loop is handed exactly that operand
  zero words           on lane, wave and tile borders, in the first and last bin, beside the pad words and five in a row, in runs of 39 .. 2057 bins that
                       end on a tile, one word short of it and one word into the next; pad counts 0, 1, 2, 3; the pad cells poisoned on input
  wide challenges      shifts, beta and gamma around every border of fr_reduce (r, 2r, 4r), per call and per string
  the operand matrix   a product whose A + beta, inv_beta and inv_gamma are edge operands; open=False
  M and the tiles      M = 1023, 1024, 1025, 2048 with n_rows below, on and above it

No test provokes a fault: every index is a word of its lookup or a pattern the rule answers with a zero term (the host twin ran it first), every cell is
below r, and only shifts, beta and gamma are unreduced."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import product_edges as pe
import product_ref as pr
from compress_ref import R
from fr_edges import E, POISON64, limbs_array
from test_compress_gpu import on_device
from test_permute_cpu import lookups_of
from test_product_gpu import POISON32, Z, d32, device_invert, same_as_host

pytestmark = pytest.mark.gpu
FORMS = [False, True]


def both(cfg, table, shift, canonical, first_wrong):
    """the device's inverse table between its guards, held to the Python expectation — first_wrong(got) names the first wrong case — and to the host twin"""
    table, shift = np.array(table), np.array(shift)                  # (the shared cases are read-only)
    got = device_invert(cfg, table, shift, canonical)
    pe.check(first_wrong(got))
    host = cfg.lookup_invert_table_host(table, shift, canonical=canonical)
    bad = np.argwhere((got != host).any(axis=-1))
    assert not len(bad), "the device differs from the host twin at (run, word) %s, %s" % (bad[0], pe.FORMS[canonical])
    return got


# ---- the inverse tables -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("bins,positions,c", [(2057, None, int.from_bytes(np.random.default_rng(8).bytes(32), "little") % R), (39, (0, 3, 4, 38), pe.WIDE_SHIFTS[6])],
                         ids=["2057-bins", "39-bins"])
def test_fr_inv_is_handed_every_edge_operand_alone(bins, positions, c, canonical):
    """one invert call: 33 operands x 15 positions, three tiles a run (2057 bins); 33 x 4, most lanes holding nothing but ones (39 bins)"""
    cfg = pe.sized_cfg(bins, 40, device=0)
    W = cfg.lookup_words()
    table, cases = pe.isolation_runs(bins, W, E, pe.BORDERS(bins) if positions is None else positions, c)
    both(cfg, table, limbs_array([c])[0], canonical, lambda got: pe.first_wrong_isolation(got, cases, W, canonical))


@pytest.mark.parametrize("canonical", FORMS)
def test_a_run_of_zero_words_only(canonical):
    for bins in (39, 2057):
        cfg = pe.sized_cfg(bins, 40, device=0)
        table, cases = pe.isolation_runs(bins, cfg.lookup_words(), [0], [0], pe.WIDE_SHIFTS[-1])
        got = both(cfg, table[0], limbs_array([pe.WIDE_SHIFTS[-1]])[0], canonical, lambda got: "%d bins, %s: a word is not the zero cell" % (bins, pe.FORMS[canonical]) if got.any() else None)
        assert got.shape == (cfg.lookup_words(), 4)


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("group", range(pe.ZERO_GROUPS))
@pytest.mark.parametrize("bins", list(pe.SIZED))
def test_zero_words_on_every_border_of_every_run_size(bins, group, canonical):
    """groups 0 .. 2: three runs, a shift of WIDE_SHIFTS each (shift_stride 4); group 3: two runs under one shift for the call (shift_stride 0)"""
    cfg = pe.sized_cfg(bins, 40, device=0)
    table, shifts, want, planted = pe.zero_pattern_case(bins, canonical, group)
    assert (table[:, bins:] == POISON64).all() and shifts.shape == ((4,) if group == 3 else (3, 4))
    got = both(cfg, table, shifts, canonical, lambda got: pe.first_wrong_word(got, want, shifts, canonical))
    assert not got[:, bins:].any() and not got[:, planted].any(), "pad words and zero words are zero cells"


# ---- the product --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("per_string", [False, True])
def test_wide_challenges_into_the_product(per_string, canonical):
    ch = pe.wide_challenge_chain(canonical, per_string)
    cfg = pe.sized_cfg(39, ch.M, device=0)
    for beta, gamma in pe.wide_challenge_pairs(per_string):
        got = same_as_host(cfg, ch.lens, ch.inputs, ch.a_idx, ch.s_idx, ch.n_rows, ch.table, beta, gamma, canonical)
        low = same_as_host(cfg, ch.lens, ch.inputs, ch.a_idx, ch.s_idx, ch.n_rows, ch.table, pe.reduced(beta), pe.reduced(gamma), canonical)
        assert np.array_equal(got["z"], low["z"]) and np.array_equal(got["open"], low["open"]), "a challenge means its value mod r"
        z, opened, ints = pr.product(lookups_of(cfg), ch.lens, ch.M, ch.inputs, ch.a_idx, ch.s_idx, ch.n_rows, ch.table, beta, gamma, canonical)
        what = "beta %#x: " % pe.int_of(beta.reshape(-1, 4)[0])
        pe.check(pe.first_wrong_z(got["z"], z, ch.n_rows, canonical, what))
        assert np.array_equal(got["open"], opened)


@pytest.mark.parametrize("canonical", FORMS)
def test_a_product_whose_every_factor_is_an_edge_operand(canonical):
    cfg = pe.sized_cfg(39, 40, device=0)
    m = pe.operand_matrix(cfg, canonical)
    B, n_rows = len(m["lens"]), m["n_rows"]
    host = cfg.lookup_product_host(m["lens"], m["inputs"], m["a_idx"], m["s_idx"], n_rows, m["table"], m["inv_beta"], m["inv_gamma"], m["beta"], m["gamma"],
                                   canonical=canonical)
    up = lambda k: (d32 if m[k].dtype == np.uint32 else on_device)(np.array(m[k]))                  # (the shared case is read-only)
    dev = [up(k) for k in ("lens", "inputs", "a_idx", "s_idx")] + [n_rows] + [up(k) for k in ("table", "inv_beta", "inv_gamma", "beta", "gamma")]
    out = Z(3, B, n_rows, 0)
    res = cfg.lookup_product(*dev, canonical=canonical, out=out.tensors())
    torch.cuda.synchronize()
    got = out.numpy()
    assert set(res) == {"z", "open"}
    pe.check(pe.first_wrong_z(got["z"], m["z"], n_rows, canonical))
    assert np.array_equal(got["z"][:, :, :n_rows + 1], host["z"][:, :, :n_rows + 1]) and np.array_equal(got["open"], m["open"]) and np.array_equal(got["open"], host["open"])
    # open=False: the same Z, the poisoned open words untouched
    out2 = Z(3, B, n_rows, 0)
    res = cfg.lookup_product(*dev, canonical=canonical, open=False, out={"z": out2.z[1]})
    torch.cuda.synchronize()
    assert set(res) == {"z"} and bool((out2.open[0] == POISON32).all()), "open was written"
    assert np.array_equal(out2.numpy()["z"], got["z"])


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("bins,M,n_rows", pe.m_border_cases())
def test_M_on_and_around_a_tile_border(bins, M, n_rows, canonical):
    cfg = pe.sized_cfg(bins, M, device=0)
    assert cfg.lookup_product_plan(4, n_rows)["tile_rows"] == 1024
    ch, z, opened = pe.m_border_chain(bins, M, n_rows, canonical)
    got = same_as_host(cfg, ch.lens, ch.inputs, ch.a_idx, ch.s_idx, n_rows, ch.table, ch.beta, ch.gamma, canonical)
    pe.check(pe.first_wrong_z(got["z"], z, n_rows, canonical, "M %d: " % M))
    assert np.array_equal(got["open"], opened)
