"""The variant matrix of tests/test_variants_gpu.py checked where no device is needed: every row's seeds reach the variant the row forces
(describe_launch of a host-only context plans the same launch), together hold every edge case of tests/fuzz_defs.py the row admits, and
are not vacuous; the generator's cases through the library's host walk against the oracle."""
import os

import numpy as np
import pytest

import halo2_regex_amd as hra
import fuzz_defs as fd
from oracle_lib import OracleDefs
from test_variants_gpu import ROWS, ROW_IDS, applicable_edges, check_describe, fr_case, make_config, _cases

THREADS = min(16, os.cpu_count() or 1)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_row_seeds_reach_the_variant_and_cover_its_edges(oracle, row):
    edges, codes, accepted, masked_nonzero = set(), set(), False, False
    planted, ds = {}, set()
    cases = _cases(row)
    if row.get("fr"):
        assert fr_case(row, cases) is not None      # fr_columns is checked on many strings of a real M (one def where the stripes form is asked for)
    for case in cases:
        ds.add(case.D)
        cfg = make_config(hra, row, case, hra.HRX_DEVICE_NONE)
        check_describe(row, cfg, case, host_only=True)        # a row whose shapes cannot reach its variant is a bug in the row
        edges |= case.edges
        o = OracleDefs(oracle, [(a, subs) for a, subs, _ in case.defs_t])
        _, omsk, ost = o.witness_batch(case.chars, case.lens, case.M, threads=THREADS)
        code = (ost & np.uint64(0xff)).astype(np.int64)
        codes |= set(code.tolist())
        if case.D == 1:
            assert not (code == 2).any()        # one def flags a row at most once: status 2 needs two defs
        if case.B > 1:
            assert (code == 0).mean() >= 1 / 3, (case.seed, np.bincount(code))
        accepted |= bool(((ost >> np.uint64(8)) & np.uint64(0xffffffff))[code == 0].any())
        masked_nonzero |= bool(omsk[code == 0].any())
        for b, p, edge in case.plants:      # a planted transition is where def 0's walk stops (the oracle's status 1: def, position)
            s = int(ost[b])
            if s & 0xff == 1 and (s >> 8) & 0xff == 0 and s >> 40 == p:
                planted[edge] = planted.get(edge, 0) + 1
    assert ds == set(range(row["shape"].d_lo, row["shape"].d_hi + 1)), sorted(ds)      # every D the row admits
    missing = applicable_edges(row) - edges
    assert not missing, sorted(missing)
    undef = applicable_edges(row) & set(fd.UNDEF_EDGES)
    assert undef <= set(planted), sorted(undef - set(planted))
    assert {0, 1, 3} | ({2} if row["shape"].d_hi >= 2 else set()) <= codes, sorted(codes)
    assert accepted and masked_nonzero


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_generator_cases_through_the_host_walk(oracle, row):
    """hrx_witness_batch_host on a host-only context (the native host walk) against the oracle, every case of the row"""
    for case in _cases(row):
        defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]
        cfg = hra.RegexVerifyConfig.configure(case.M, defs, device=hra.HRX_DEVICE_NONE)
        orec, omsk, ost = OracleDefs(oracle, [(a, subs) for a, subs, _ in case.defs_t]).witness_batch(case.chars, case.lens, case.M, threads=THREADS)
        grec, gmsk, gst = cfg.witness_batch_host(case.chars, case.lens)
        assert np.array_equal(gst, ost), case.seed
        ok = (ost & np.uint64(0xff)) == 0
        assert np.array_equal(grec[ok], orec[ok]) and np.array_equal(gmsk[ok], omsk[ok]), case.seed


def test_cases_are_deterministic_per_seed():
    sh = fd.Shape(1, 3, ids=("ids_63",))
    a, b = fd.make_case(7, sh), fd.make_case(7, sh)
    assert a.defs_t[0][0] == b.defs_t[0][0] and a.defs_t[0][1] == b.defs_t[0][1]
    assert np.array_equal(a.chars, b.chars) and np.array_equal(a.lens, b.lens) and a.edges == b.edges
    assert not np.array_equal(fd.make_case(8, sh).lens, a.lens) or fd.make_case(8, sh).M != a.M


@pytest.mark.parametrize("seed", [0, 2, 6, 8])
def test_substring_ids_past_the_byte_slot_leave_the_byte_table(seed):
    """A BYTE-table slot holds 6 bits of substring id (csrc/hrx_defs.cpp build_byte_table): the same big DFA with ids up to 62 / 63 takes the BYTE
    table when it is forced, with ids up to 64 / 65 the planner falls back to another table (and says so in describe_launch)."""
    flags = {"flags": 0x2000 | 0x8000000}
    fit = fd.make_case(seed, fd.Shape(1, 1, "big", ids=("ids_62", "ids_63")))
    past = fd.make_case(seed, fd.Shape(1, 1, "big", ids=("ids_64", "ids_65")))
    assert fit.defs_t[0][0] == past.defs_t[0][0]                          # the same DFA
    assert {"ids_62", "ids_63"} & fit.edges and {"ids_64", "ids_65"} & past.edges
    byte = r"witness_pm_kernel<1, false, false, false, false, true>"
    import re
    assert re.search(byte, make_config(hra, flags, fit, hra.HRX_DEVICE_NONE).describe_launch(fit.B, layout=1))
    assert not re.search(byte, make_config(hra, flags, past, hra.HRX_DEVICE_NONE).describe_launch(past.B, layout=1))
