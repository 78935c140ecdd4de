"""What tests/test_caller_conditions_gpu.py rests on, checked without a device: the cases it picks per row reach the row's variant and have the shapes the
alignment tests are about; the decoy of the side-stream tests (the batch in reversed string order) differs from the batch on at least half of the strings,
in what the oracle says about them; every batch of the long-lived-context sequence still holds strings of status 0, 1 and 3 and an accepted one that
reveals something; the helpers that build the decoys are their own inverses; include/hrx.h states the alignment rules the allocator hands out."""
import os

import numpy as np
import pytest

import caller_conditions as cc
import halo2_regex_amd as hra
from oracle_lib import ROOT, OracleDefs
from test_extract_cpu import batch
from test_match_cpu import rle_masked
from test_variants_gpu import check_describe, make_config

THREADS = min(16, os.cpu_count() or 1)
ROWS = cc.all_rows()
ROW_IDS = [r["id"] for r in ROWS]
_EXPECT = {}


def expected(oracle, key, case):
    if key not in _EXPECT:
        o = OracleDefs(oracle, [(a, subs) for a, subs, _ in case.defs_t])
        _EXPECT[key] = o.witness_batch(case.chars, case.lens, case.M, threads=THREADS)
    return _EXPECT[key]


def _describe(row, case):
    check_describe(row, make_config(hra, row, case, hra.HRX_DEVICE_NONE), case, host_only=True)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_alignment_cases_reach_the_variant_and_have_the_shapes(row):
    cases, fr_seed = cc.alignment_cases(row)
    assert 2 <= len(cases) <= 3 and len({c.seed for c in cases}) == len(cases)
    assert any(c.B % 64 for c in cases)
    admits_odd = row["id"] != cc.CHUNK_ROW_ID and row["shape"].m in ("any", "odd8")
    assert any(c.M % 8 for c in cases) == admits_odd, [c.M for c in cases]
    assert (fr_seed is not None) == bool(row.get("fr")) and (fr_seed is None or fr_seed in [c.seed for c in cases])
    for case in cases:
        _describe(row, case)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_the_decoy_bites_on_every_side_stream_case(oracle, row):
    """status word or masked rows of string b differ from those of string B - 1 - b for at least half of all b: a launch that read the decoy cannot pass"""
    case = cc.stream_case(row)
    assert case.B % 64 and case.B >= 63
    _describe(row, case)
    _, omsk, ost = expected(oracle, (row["id"], case.seed), case)
    assert cc.decoy_bites(ost, omsk) >= 0.5, (row["id"], case.seed, cc.decoy_bites(ost, omsk))
    if row["id"] in cc.SCRATCH_ROWS:      # the handover's second call: another selection, no larger than the first
        sel2 = cc.handover_selection(case.B)
        assert 1 <= len(sel2) <= case.B and len(sel2) == case.B - 1 and not np.array_equal(sel2, np.arange(len(sel2)))


@pytest.mark.parametrize("D", [1, 2, 3])
def test_the_decoy_bites_on_the_match_case(oracle, D):
    case = cc.match_case(D)
    assert case.B == 129 and case.D == D
    _, omsk, ost = expected(oracle, ("match", D), case)
    assert cc.decoy_bites(ost, omsk) >= 0.5
    ecnt, _ = rle_masked(omsk, case.lens, ost)
    code = ost & np.uint64(0xff)
    assert {0, 1, 3} <= set(code.tolist()) and max(ecnt) >= 1
    assert max(ecnt) > cc.MATCH_SPANS or D > 0          # (more runs than the cap is welcome, not required)


def test_the_decoy_bites_on_the_staging_batch():
    bt = batch("stress256").prefix(129)
    differs = (bt.ost != bt.ost[::-1]) | (np.array(bt.ecnt) != np.array(bt.ecnt)[::-1]) | (bt.lens != bt.lens[::-1])
    assert differs.mean() >= 0.5
    assert (bt.lens <= bt.chars.shape[1]).all()          # (every string fits its slot: the ragged and the string-major source hold the same strings)


@pytest.mark.parametrize("row_id", cc.SEQUENCE_ROWS)
def test_every_batch_of_the_sequence_is_a_real_one(oracle, row_id):
    """the selections are not vacuous: status 0, 1 and 3 and an accepted string that reveals something in every batch of 64 strings or more; the one-string
    batch IS such an accepted string; the step to the fourth batch is beyond reserve()'s 1.25 x headroom"""
    row = cc.row_of(row_id)
    case = cc.sequence_case(row)
    _, omsk, ost = expected(oracle, ("sequence", row_id), case)
    sizes = cc.sequence_sizes(row, case)
    assert len(sizes) == 7 and sizes[:3] == (129, 1, 65) and sizes[4:] == (64, 129, 0) and sizes[3] >= 320 and sizes[3] > 1.25 * 129 and case.B >= sizes[3]
    if sizes[3] == case.B:
        _describe(row, case)
    code = ost & np.uint64(0xff)
    good = cc.good_strings(ost, omsk)
    accepted = (((ost >> np.uint64(8)) & np.uint64(0xffffffff)) != 0)[good]
    assert accepted.all() if row_id != cc.CHUNK_ROW_ID else not accepted.any()          # (the lever definitions of the chunked row accept nothing)
    seen = set()
    for k, n in enumerate(sizes):
        sel = cc.selection(case, ost, omsk, k, n)
        assert len(sel) == n and len(set(sel.tolist())) == n and (n == 0 or sel.max() < case.B)
        seen.add(tuple(sel.tolist()))
        if n == 1:
            assert good[sel[0]]
        elif n:
            assert {0, 1, 3} <= set(code[sel].tolist()), (row_id, k, n, np.bincount(code[sel].astype(np.int64)))
            assert good[sel].any(), (row_id, k, n)
    assert len(seen) == 7          # (the two batches of 129 differ)


def test_decoy_helpers_are_their_own_inverses():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    chars = rng.integers(1, 255, (70, 48)).astype(np.uint8)
    pm = hra.chars_to_position_major(torch.from_numpy(chars))
    assert np.array_equal(cc.pm_chars_to_string_major(pm, 70, 48).numpy(), chars)
    lens = rng.integers(0, 49, 70)
    lens[5] = 0
    offsets = np.concatenate(([3], 3 + np.cumsum(lens))).astype(np.int64)
    values = np.full(-(-int(offsets[-1]) // 16) * 16 + 16, 0xAA, np.uint8)
    values[3:int(offsets[-1])] = np.concatenate([chars[b, :lens[b]] for b in range(70)])
    rv, ro = cc.reversed_ragged(torch, torch.from_numpy(values), torch.from_numpy(offsets))
    assert rv.shape == (len(values),) and ro.shape == (71,) and int(ro[0]) == 3 and int(ro[-1]) == int(offsets[-1])
    for b in range(70):
        assert bytes(rv.numpy()[int(ro[b]):int(ro[b + 1])]) == bytes(chars[69 - b, :lens[69 - b]])
    bv, bo = cc.reversed_ragged(torch, rv, ro)
    assert np.array_equal(bv.numpy(), values) and np.array_equal(bo.numpy(), offsets)


def test_the_header_states_the_alignments_the_allocator_hands_out():
    text = " ".join(open(os.path.join(ROOT, "include", "hrx.h")).read().split())
    assert "chars, records, masked and every * record plane / row stripe 16 bytes, status 8 bytes, lens 4 bytes" in text
    a = cc.MIN_ALIGN
    assert (a["chars"], a["records"], a["masked"], a["plane"], a["status"], a["lens"]) == (16, 16, 16, 16, 8, 4)
    assert (a["values"], a["chars_pm"], a["cells"], a["offsets"], a["spans"], a["workspace"], a["sel"], a["order"], a["span_counts"]) == (16, 16, 16, 8, 8, 8, 4, 4, 4)
    assert cc.GUARD == 4096
