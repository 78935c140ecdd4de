"""What tests/fr_cases.py claims, asserted from the oracle alone (no GPU), and the host-side twins of the field-cell kernel on its cases:
hrx_witness_columns_host (csrc/hrx_fill.cpp) and hrx_fr_from_u64 (csrc/hrx_fr.h) on state values above 255, which no other test gives them."""
import re

import numpy as np
import pytest

import halo2_regex_amd as hra
import fr_cases as fc
from oracle_lib import OracleDefs

M_SWEEP = 72


def _mont(v):
    return (int(v) << 256) % fc.FR_MODULUS


@pytest.fixture(scope="module", params=[1, 2], ids=["D1", "D2"])
def sweep(request, oracle):
    D = request.param
    defs_t = fc.sweep_defs(D)
    o = OracleDefs(oracle, defs_t)
    chars, lens = fc.sweep_batch(fc.SWEEP_L if D == 1 else fc.SWEEP_L2)
    orec, omsk, ost = o.witness_batch(chars, lens, M_SWEEP)
    return dict(D=D, defs_t=defs_t, o=o, chars=chars, lens=lens, orec=orec, omsk=omsk, ost=ost,
                cols=fc.expected_columns(orec, omsk, chars, lens, M_SWEEP, D))


def test_sweep_batch_holds_every_state_value(sweep):
    D, cols, lens = sweep["D"], sweep["cols"], sweep["lens"]
    L = fc.SWEEP_L if D == 1 else fc.SWEEP_L2
    assert not (sweep["ost"] & np.uint64(0xff)).any()                                  # status 0 everywhere
    assert sweep["chars"].shape == (40, 80) and int((lens == 0).sum()) == 1 and int((lens == M_SWEEP).sum()) >= 16
    assert set(int(x) for x in lens[1:32:2]) == set(range(M_SWEEP - 8, M_SWEEP))
    for d in range(D):
        states = np.unique(cols[2 + 4 * d])
        assert np.array_equal(states, np.arange(L + 2))                                # all of 0..L and the dummy L + 1
        assert int((states >= 256).sum()) == L + 2 - 256                               # 1791 of them for L = 2045
        assert set(np.unique(cols[3 + 4 * d]).tolist()) == {0, d + 1}                  # ids
        assert cols[4 + 4 * d].sum() > 200 and cols[5 + 4 * d].sum() > 200             # start and end flags
    assert int((cols[2 + 4 * D] != 0).sum()) > 1000                                    # nonzero masked rows
    assert set(np.unique(cols[3 + 4 * D]).tolist()) == set(range(D + 1))
    assert cols.max() == L + 1 and cols.min() == 0


def test_largest_definition_a_config_takes():
    mk = lambda L: [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs in [fc.sweep_def(L)]]
    cfg = hra.RegexVerifyConfig.configure(M_SWEEP, mk(fc.SWEEP_L), device=hra.HRX_DEVICE_NONE)
    assert cfg.table_bytes() == 2048 * 1024
    with pytest.raises(hra.HrxError):
        hra.RegexVerifyConfig.configure(M_SWEEP, mk(fc.SWEEP_L + 1), device=hra.HRX_DEVICE_NONE)


def test_expected_columns_equal_match_substrs_on_the_sweep(sweep):
    ref = fc.columns_of_match_substrs(sweep["o"], sweep["chars"], sweep["lens"], M_SWEEP, range(40))
    assert np.array_equal(ref, sweep["cols"])


def _host_cfg(defs_t, M):
    defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs in defs_t]
    return hra.RegexVerifyConfig.configure(M, defs, device=hra.HRX_DEVICE_NONE)


def test_host_walk_and_host_columns_on_states_above_255(sweep):
    D, chars, lens, cols = sweep["D"], sweep["chars"], sweep["lens"], sweep["cols"]
    cfg = _host_cfg(sweep["defs_t"], M_SWEEP)
    d0, d3 = cfg.describe_launch(40, layout=0), cfg.describe_launch(40, layout=3)
    assert re.match(r"hrx::witness_kernel<%d, (true|false), true>" % D, d0), d0      # witness_kernel<D, ALIGNED, GTAB>: the global-table kernel
    assert d3.startswith("hrx::witness_pm_kernel<%d, true," % D), d3
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    assert np.array_equal(st, sweep["ost"]) and np.array_equal(rec, sweep["orec"]) and np.array_equal(msk, sweep["omsk"])      # the host walk equals the oracle
    got = hra.witness_columns_host(chars, lens, sweep["orec"], sweep["omsk"], M_SWEEP, D)
    assert np.array_equal(got.astype(np.int64), cols)
    part = hra.witness_columns_host(chars, lens, sweep["orec"], sweep["omsk"], M_SWEEP, D, b_begin=7, b_count=21)
    assert np.array_equal(part.astype(np.int64), cols[:, 7:28])
    rpm, mpm = fc.to_position_major(sweep["orec"], sweep["omsk"])
    for src, kw in ((chars, {}), (fc.chars_position_major(chars), dict(chars_pm_stride=chars.shape[1]))):
        got = hra.witness_columns_host(src, lens, rpm, mpm, M_SWEEP, D, position_major=True, B=40, **kw)
        assert np.array_equal(got.astype(np.int64), cols)
        part = hra.witness_columns_host(src, lens, rpm, mpm, M_SWEEP, D, b_begin=7, b_count=21, position_major=True, B=40, **kw)
        assert np.array_equal(part.astype(np.int64), cols[:, 7:28])


def test_to_position_major_is_the_layout_of_the_header():
    """fc.to_position_major against the library's own inverse and its one-string gather, across a block border"""
    rng = np.random.default_rng(2)
    for B, M, D in ((40, 72, 2), (65536 + 9, 5, 1), (7, 13, 3)):
        rec = rng.integers(0, 2 ** 32, (B, M, D), dtype=np.uint64).astype(np.uint32)
        msk = rng.integers(0, 65536, (B, M)).astype(np.uint16)
        rpm, mpm = fc.to_position_major(rec, msk)
        r2, m2 = hra.position_major_to_string_major(rpm, mpm, B, M, D)
        assert np.array_equal(r2, rec) and np.array_equal(m2, msk)
        for b in (0, B - 1, min(B - 1, 65536)):
            r1, m1 = hra.rows_of_string_position_major(rpm, mpm, B, M, D, b)
            assert np.array_equal(r1, rec[b]) and np.array_equal(m1, msk[b])


def test_fr_from_u64_equals_the_table_up_to_the_largest_state():
    for canonical in (False, True):
        t = fc.lut(canonical)
        got = np.array([hra.fr_from_u64(v, canonical=canonical) for v in range(2047)], np.uint64)
        assert fc.first_difference(got[None, None], t[None, None, :2047]) is None
    for v in (0, 1, 255, 256, 2046, 65535):
        assert sum(int(x) << (64 * i) for i, x in enumerate(fc.lut(False)[v])) == _mont(v)
    assert fc.cells_of(np.array([[3, 2046]]), True).tolist() == [[[3, 0, 0, 0], [2046, 0, 0, 0]]]


def test_the_comparison_reports_one_wrong_limb():
    cols = np.arange(2 * 3 * 5).reshape(2, 3, 5) + 250
    want = fc.cells_of(cols, False)
    assert fc.first_difference(want.copy(), want) is None
    for c, b, r, k in ((0, 0, 0, 0), (1, 2, 4, 3), (1, 0, 3, 2)):
        bad = want.copy()
        bad[c, b, r, k] ^= np.uint64(1 << 40)
        msg = fc.first_difference(bad, want)
        assert msg is not None and msg.startswith("column %d string %d row %d limb %d:" % (c, b, r, k)) and "(1 cells differ)" in msg
    # ... and one wrong limb of one table entry
    t = fc.lut(False).copy()
    t[1234, 2] += np.uint64(1)
    msg = fc.first_difference(fc.cells_of(np.array([[[7, 1234, 9]]]), False, table=t), fc.cells_of(np.array([[[7, 1234, 9]]]), False))
    assert msg is not None and msg.startswith("column 0 string 0 row 1 limb 2:")
    assert fc.first_difference(want[:, :2], want) is not None       # a shape mismatch is a difference


@pytest.mark.parametrize("M", fc.EDGE_MS)
def test_row_count_edge_batches(oracle, M):
    o = OracleDefs.from_files(oracle, fc.CFG_A)
    chars, lens, stride = fc.edge_batch(M)
    assert stride > M and stride % 16 == 0 and chars.shape == (5, stride) and lens.tolist() == [0, 1, M - 1, M, M // 2]
    orec, omsk, ost = o.witness_batch(chars, lens, M)
    assert not (ost & np.uint64(0xff)).any()
    cols = fc.expected_columns(orec, omsk, chars, lens, M, 2)
    assert np.array_equal(fc.columns_of_match_substrs(o, chars, lens, M, range(5)), cols)
    ids = set(np.unique(cols[3 + 4 * 2]).tolist())
    assert ids == ({0} if M < 12 else {0, 2} if M < 70 else {0, 1, 2})                 # the planted matches are revealed where they fit
    if M >= 31:
        assert all(cols[2 + 4 * 2, b].any() and cols[4 + 4 * 1, b].any() and cols[5 + 4 * 1, b].any() for b in (2, 3, 4))
        assert cols[5 + 4 * 1, 2, M - 3] == 1                                           # (even strings: the match ends at the string's last byte)


def _defcount_configs():
    import test_parity_gpu as tp
    return {"D4": (tp.CFG_D4, 0.5), "D5": (tp.CFG_D5, 0.5), "D6": (tp.CFG_D6, 0.5), "D7": (tp.CFG_D7, 0.0), "D8": (tp.CFG_D8, 0.0), "D13": (tp.CFG_D13, 0.0),
            "D12": (tp.CFG_123 + tp.HDR + tp.NOSUB(tp.CFG_123 + tp.HDR), 0.0)}


@pytest.mark.parametrize("name", ["D4", "D5", "D6", "D7", "D8", "D13", "D12"])
def test_def_count_batches(oracle, name):
    names, share = _defcount_configs()[name]
    o = OracleDefs.from_files(oracle, names)
    D = o.D
    assert D == int(name[1:])
    chars, lens = fc.defcount_batch(names)
    assert chars.shape == (70, 80)
    orec, omsk, ost = o.witness_batch(chars, lens, 72)
    ok = np.nonzero((ost & np.uint64(0xff)) == 0)[0]
    assert len(ok) >= 70 * max(share, 2 / 3), (name, len(ok))
    cols = fc.expected_columns(orec, omsk, chars, lens, 72, D)
    assert np.array_equal(fc.columns_of_match_substrs(o, chars, lens, 72, ok), cols[:, ok])
    # as many different state columns as the config has different DFAs (regex3 and the `from:` header definition count as one: their walks part only on a
    # `from:` line, which both flag — status 2): a column written in another def's place is seen
    distinct = len({cols[2 + 4 * d][ok].tobytes() for d in range(D)})
    assert distinct == {"D4": 3, "D5": 5, "D6": 5, "D7": 6, "D8": 5, "D13": 6, "D12": 5}[name]
    if name not in ("D7", "D13"):      # (their status-0 strings end before anything is revealed)
        assert (cols[2 + 4 * D][ok] != 0).sum() > 400 and len(np.unique(cols[3 + 4 * D][ok])) >= 3


def test_big_batch_and_its_sample(oracle):
    sample = fc.big_sample()
    assert len(sample) >= 200 and {65535, 65536, 65399, 65400, 65699, 65700, 65537, fc.BIG_B - 2, fc.BIG_B - 1, 29999, 30000, 62767, 62768, 65799, 65800} <= set(sample)
    for names, alphabet, D in ((fc.CFG_1, None, 1), (fc.CFG_A, None, 2), (None, fc.BIG_SWEEP_BYTES, 1)):
        o = OracleDefs.from_files(oracle, names) if names else OracleDefs(oracle, [fc.sweep_def(fc.BIG_SWEEP_L)])
        chars, lens = fc.big_batch(alphabet)
        assert chars.shape == (fc.BIG_B, 16) and fc.BIG_B == 65536 + 300
        orec, omsk, ost = o.witness_batch(chars, lens, fc.BIG_M, threads=8)
        assert not (ost & np.uint64(0xff)).any()
        cols = fc.expected_columns(orec, omsk, chars, lens, fc.BIG_M, D)
        assert np.array_equal(fc.columns_of_match_substrs(o, chars, lens, fc.BIG_M, sample), cols[:, sample])
        for side in (slice(0, 65536), slice(65536, None)):
            assert set(np.unique(lens[side]).tolist()) == set(range(9))
            assert len(np.unique(cols[2, side])) >= 9                              # states beyond the first and the dummy
            if alphabet is None:
                assert any(b"@x." in bytes(r) for r in chars[side][:300, :8])
                assert not cols[2 + 4 * D, side].any()      # regex1 / regex2 reveal nothing within 8 rows: their public parts begin after 21 / 10 literal bytes
            else:
                assert (cols[2 + 4 * D, side] != 0).sum() > 50 and cols[4, side].any() and cols[5, side].any()
        # neighbours differ: a string read from the other block, or from the next slot, is seen
        assert (cols[:, 1:] != cols[:, :-1]).any(axis=(0, 2)).all()


def test_block_border_batch_of_19_rows(oracle):
    """The 19-row batch behind string 65536: masked octets 1 and 2 and chars group 1 are live in the second block, and a kernel that took another string count
    than nb = 300 for that block (here nb - 1, which stays inside the buffers) would read other values in every short request"""
    o = OracleDefs(oracle, [fc.sweep_def(fc.BIG_SWEEP_L)])
    chars, lens = fc.tall_batch()
    B, M = fc.BIG_B, fc.TALL_M
    assert chars.shape == (B, 32) and M == 19 and lens.max() == M and all(lens[b] == M for b in fc.TALL_PLANTED)
    orec, omsk, ost = o.witness_batch(chars, lens, M, threads=8)
    assert not (ost & np.uint64(0xff)).any()
    cols = fc.expected_columns(orec, omsk, chars, lens, M, 1)
    sample = fc.big_sample()
    assert len(sample) >= 200 and set(fc.TALL_PLANTED) - {fc.BIG_B - 2} <= set(sample)
    assert np.array_equal(fc.columns_of_match_substrs(o, chars, lens, M, sample), cols[:, sample])
    second = slice(fc.PM_BLOCK, None)
    assert set(np.unique(lens[second]).tolist()) == set(range(M + 1))
    assert cols[6, second, 8:16].any() and cols[6, second, 16].any() and cols[7, second, 8:].any() and cols[1, second, 16].any()
    assert cols[4, second].any() and cols[5, second].any() and (cols[:, 1:] != cols[:, :-1]).any(axis=(0, 2)).all()
    rpm, mpm = fc.to_position_major(orec, omsk)
    cpm = fc.chars_position_major(chars)
    same, less = (lambda nb: nb), (lambda nb: nb - 1)
    for b0, n in fc.BIG_SHORT:
        seen_m = seen_c = False
        for b in range(max(b0, fc.PM_BLOCK), b0 + n):
            for r in range(M):
                assert fc.gather_with_nb(mpm, 8, 3, B, b, r, same) == omsk[b, r] and fc.gather_with_nb(cpm, 16, 2, B, b, r, same) == chars[b, r]
                seen_m |= bool(fc.gather_with_nb(mpm, 8, 3, B, b, r, less) != omsk[b, r])
                seen_c |= bool(r < lens[b] and fc.gather_with_nb(cpm, 16, 2, B, b, r, less) != chars[b, r])
        assert seen_m and seen_c, (b0, n, seen_m, seen_c)


def test_out_of_contract_batch(oracle):
    o = OracleDefs.from_files(oracle, fc.CFG_A)
    chars, lens = fc.bad_batch()
    orec, omsk, ost = o.witness_batch(chars, lens, 72)
    code = ost & np.uint64(0xff)
    assert tuple(np.nonzero(code)[0]) == fc.BAD_STRINGS and code[3] == 3 and code[40] == 3 and code[9] == 1
    assert lens[3] == 73 and lens[40] == 73 and chars.shape[1] > 73
