"""The carry scenarios of tests/carry_defs.py where no device is needed: a row-by-row transcription of the reveal mask (src/lib.rs:593-764) over the
oracle's substr_id / start_enable / end_enable columns equals the oracle's masked columns on every scenario string (the independent reference for
this one operation; the oracle stays the judge of the rest of the row); the batches the GPU tests launch are what they claim (long confirmed and
taken-back ranges, every border opened at and resolved at, the expected status codes); a walker that left out the end-mask fix-up or the chunk
repair gets every take-back / carry-in scenario wrong; and the library's host walk and the lane simulation on the same batches."""
import os

import numpy as np
import pytest

import carry_defs as cd
import halo2_regex_amd as hra
from oracle_lib import OracleDefs
from test_match_cpu import rle_masked
from test_lane_sim import SimDefs, sim      # noqa: F401  (the fixture)

THREADS = min(16, os.cpu_count() or 1)


def py_masks(sid, st, en, M):
    """lib.rs:598-745 on integers, row by row; sid has M entries, st and en M + 1 (assigned_is_start / assigned_is_end)"""
    sm, em, last = [0] * M, [0] * M, 0
    for i in range(M):                                   # lib.rs:598-645
        changed = (0 if i == 0 else sid[i - 1]) != sid[i]
        if st[i] and changed:
            last = 1
        if (not st[i]) and en[i] and changed:
            last = 0
        sm[i] = last
    last = 0
    for i in range(M):                                   # lib.rs:663-714
        pre = 0 if i == 0 else sid[M - i]
        changed = pre != sid[M - 1 - i]
        if en[M - i] and changed:
            last = 1
        if (not en[M - i]) and st[M - i] and changed:
            last = 0
        em[M - 1 - i] = last
    return [a & b for a, b in zip(sm, em)]               # lib.rs:740-745


def _oracle(oracle, case):
    return OracleDefs(oracle, [(a, subs) for a, subs, _ in case.defs_t])


def _distinct(case):
    """one index per distinct string of the batch"""
    seen, out = set(), []
    for b in range(case.B):
        key = bytes(case.chars[b, :case.lens[b]])
        if key not in seen:
            seen.add(key)
            out.append(b)
    return out


def _check_masks(o, case, python_rows):
    """numpy and (on python_rows strings) the row-by-row transcription against the oracle's masked columns; returns the per-string columns"""
    M, out = case.M, {}
    for k, b in enumerate(_distinct(case)):
        if case.want[b]:
            continue
        text = case.chars[b, :case.lens[b]]
        cols, sid, st, en = cd.columns(o, text, M)
        assert cols["rc"] == 0, case.names[b]
        ch = np.zeros(M, np.int64)
        ch[:len(text)] = text
        mask = cd.reveal_mask(sid, st, en)
        assert np.array_equal(mask * ch, cols["masked_char"].astype(np.int64)), case.names[b]
        assert np.array_equal(mask * sid, cols["masked_substr_id"].astype(np.int64)), case.names[b]
        if python_rows is None or k % python_rows == 0:
            assert py_masks(sid.tolist(), st.tolist(), en.tolist(), M) == mask.tolist(), case.names[b]
        out[b] = (sid, st, en, mask)
    return out


@pytest.mark.parametrize("form", sorted(cd.FORMS), ids=sorted(cd.FORMS))
def test_transcription_equals_the_oracle_on_every_scenario(oracle, form):
    case = cd.scenario_batch(cd.WITNESS_M, chunk=cd.FORCED_CHUNK, **cd.FORMS[form])
    cols = _check_masks(_oracle(oracle, case), case, None)
    assert len(cols) > 300


def _claims(oracle, case, chunk):
    """the conditions of the module docstring on one batch; prints the range metric"""
    M = case.M
    o = _oracle(oracle, case)
    _, omsk, ost = o.witness_batch(case.chars, case.lens, M, threads=THREADS)
    code = (ost & np.uint64(0xff)).astype(np.int64)
    assert np.array_equal(code, case.want), [(case.names[b], int(code[b])) for b in np.flatnonzero(code != case.want)[:5]]
    opened, resolved, longest = set(), set(), {"confirmed": 0, "taken_back": 0}
    for b in range(case.B):
        if code[b]:
            continue
        for a, r, kind in case.ranges[b]:
            m = omsk[b]
            if kind == "confirmed":
                assert m[a:r + 1].all() and not m[r + 1:r + 2].any() and (a == 0 or not m[a - 1]), (case.names[b], a, r)
            else:
                assert not m[a:min(r, M)].any(), (case.names[b], a, r)
            opened.add(a)
            resolved.add(r)
            longest[kind] = max(longest[kind], min(r, M) - a)
    want = cd.borders(M, chunk)
    assert not [p for p in want if p <= M - 1 and p not in opened], "no range opens there"
    assert not [p for p in want if p >= 1 and p not in resolved], "no range is resolved there"
    assert min(longest.values()) >= M - 80, longest
    metric = [0, 0, 0]
    cols = _check_masks(o, case, 97)
    for b, (sid, st, en, _) in cols.items():
        metric = [max(x, y) for x, y in zip(metric, cd.range_metric(sid, st, en, int(case.lens[b])))]
    print("M=%d chunk=%d B=%d: longest optimistic range confirmed %d, taken back by an event %d, by the string's end %d" % ((M, chunk, case.B) + tuple(metric)))
    assert min(metric) >= M - 80 - cd.TILE, metric      # (the metric leaves out the rows of the resolving event's own tile)
    return cols


OTHER_M = [(320, cd.FORCED_CHUNK, "variants"), (1001, cd.FORCED_CHUNK, "variants"), (2000, cd.FORCED_CHUNK, "variants"),      # the variant rows' other row counts
           (321, cd.FORCED_CHUNK, "variants"), (1000, cd.FORCED_CHUNK, "variants"), (2040, cd.FORCED_CHUNK, "variants"), (2047, cd.FORCED_CHUNK, "variants")]


@pytest.mark.parametrize("M,chunk,kind", cd.CHUNKED + OTHER_M, ids=["%d-%s" % (m, k) for m, _, k in cd.CHUNKED + OTHER_M])
def test_batches_are_what_they_claim(oracle, M, chunk, kind):
    _claims(oracle, cd.scenario_batch(M, chunk=chunk, lean=M > 8192), chunk)


@pytest.mark.parametrize("form", ["second", "three", "big", "reduced", "seven_wide"] + list(cd.SM_ROW_FORMS))
def test_forms_are_what_they_claim(oracle, form):
    case = cd.scenario_batch(cd.WITNESS_M, chunk=cd.FORCED_CHUNK, **cd.FORMS[form])
    _claims(oracle, case, cd.FORCED_CHUNK)
    if cd.FORMS[form]["D"] >= 2:      # two defs flag one row behind a long pending range: status 2 at the row of the byte that is s to both, the range opened M - 80 rows or more in front of it
        b = case.names.index("overlap")
        text = case.chars[b, :case.lens[b]]
        both, opened = int(np.flatnonzero(text == cd.BOTH)[0]), int(np.flatnonzero(text == cd.LEVERS[0][1])[0])
        st = int(_oracle(oracle, case).witness_batch(case.chars[b:b + 1], case.lens[b:b + 1], case.M)[2][0])
        assert st & 0xff == 2 and st >> 40 == both and both - opened >= case.M - 80, (hex(st), opened, both)


SM_ROWS = ("sm-three-defs-loader-walker", "sm-multi-pass-copy-combine", "sm-class-wide-transpose", "sm-class-wide-groups-transpose", "sm-multi-pass-merge-transpose",
           "sm-multi-pass-combine-transpose", "sm-via-pm-half-defs", "sm-one-wave-gs16", "sm-class-wide-transpose-two-blocks", "sm-copy-combine-two-blocks")


def test_the_string_major_rows_run_checked_forms_at_checked_row_counts():
    """the rows of the variant matrix for string-major outputs of three and more defs: the lever batches tests/test_carry_gpu.py gives them are forms and row counts
    this file checks, at row counts the row's shape admits, and describe_launch of a host-only context names the row's variant for every one of them; the lever
    table holds twelve defs of six bytes each that nothing else uses"""
    import fuzz_defs as fd
    from test_variants_gpu import ROWS, check_describe, make_config
    own = [c for lv in cd.LEVERS for c in lv]
    assert len(cd.LEVERS) == 12 and len(set(own)) == 72
    assert not set(own) & ({cd.BOTH, cd.UNDEF, cd.PADB} | set(cd.SECOND) | set(range(cd.CLASS0, cd.CLASS0 + 40)))
    checked_m = {cd.WITNESS_M} | {m for m, _, kind in OTHER_M if kind == "variants"}
    rows = [r for r in ROWS if r["id"] in SM_ROWS]
    assert len(rows) == len(SM_ROWS)
    for row in rows:
        sh = row["shape"]
        for M in cd.row_ms(sh):
            assert M in checked_m and (M % 8 != 0 if sh.m == "odd8" else M % 16 == 8 if sh.m == "m8x" else M % 8 == 0 if sh.m in ("m8", "m16") else True), (row["id"], M)
            for D in sorted({sh.d_lo, sh.d_hi}):
                form = cd.row_form(sh, D)
                assert form in cd.FORMS.values(), (row["id"], form)
                case = cd.scenario_batch(M, chunk=cd.FORCED_CHUNK, min_batch=sh.min_batch, **form)
                assert case.B >= sh.min_batch and (sh.min_batch < cd.BLOCK_BATCH or case.B % fd.PM_BLOCK % 64)      # (two blocks: the last group of the second is partial)
                check_describe(row, make_config(hra, row, case, hra.HRX_DEVICE_NONE), case, host_only=True)


def test_a_walker_without_the_fix_or_the_repair_fails_every_scenario(oracle):
    """liveness: with the fix-ups left out (pending rows keep end_mask = 1) every taken-back range of more than a tile differs from the truth, and with
    start_mask = 0 at every 256-row border every confirmed range that crosses one does"""
    case = cd.scenario_batch(cd.WITNESS_M, chunk=cd.FORCED_CHUNK, D=2)
    cols = _check_masks(_oracle(oracle, case), case, 97)
    n_fix = n_rep = 0
    for b, (sid, st, en, mask) in cols.items():
        for a, r, kind in case.ranges[b]:
            if kind == "taken_back" and min(r, case.M) // cd.TILE > a // cd.TILE:
                assert not np.array_equal(cd.reveal_mask(sid, st, en, no_fix=True), mask), case.names[b]
                n_fix += 1
            if kind == "confirmed" and r // cd.FORCED_CHUNK > a // cd.FORCED_CHUNK:
                assert not np.array_equal(cd.reveal_mask(sid, st, en, chunk_reset=cd.FORCED_CHUNK), mask), case.names[b]
                n_rep += 1
        assert np.array_equal(cd.reveal_mask(sid, st, en, no_fix=True) | mask, cd.reveal_mask(sid, st, en, no_fix=True))      # (leaving the fix out only ever reveals more)
    assert n_fix > 100 and n_rep > 50, (n_fix, n_rep)
    chunks = cd.WITNESS_M // cd.FORCED_CHUNK
    for mk in (cd.all_repair_batch, cd.no_repair_batch):
        for D in (1, 3):
            c = mk(cd.WITNESS_M, 64, D=D)
            o = _oracle(oracle, c)
            cols = _check_masks(o, c, 3)                 # (the distinct strings)
            assert c.B == 64 and not c.want.any()
            items = sum(len(cd.repair_items(*cd.columns(o, c.chars[b, :c.lens[b]], c.M)[1:], int(c.lens[b]), cd.FORCED_CHUNK)) for b in range(c.B))
            if mk is cd.no_repair_batch:
                assert items == 0
                assert not any((cd.reveal_mask(sid, st, en, chunk_reset=cd.FORCED_CHUNK) != mask).any() for sid, st, en, mask in cols.values())
                continue
            assert items == chunks * c.B                 # the repair list's capacity: every chunk of every string, the first included
            for sid, st, en, mask in cols.values():      # chunk 0 is wrong without the fix, chunks 2 .. without the repair (chunk 1 holds the second start: queued for its carry-in)
                assert (cd.reveal_mask(sid, st, en, no_fix=True) != mask)[:cd.FORCED_CHUNK].any()
                wrong = cd.reveal_mask(sid, st, en, chunk_reset=cd.FORCED_CHUNK) != mask
                assert all(wrong[c0:c0 + cd.FORCED_CHUNK].any() for c0 in range(2 * cd.FORCED_CHUNK, cd.WITNESS_M, cd.FORCED_CHUNK))
    # (a batch of confirmed ranges only stays one item per string below the capacity: chunk 0 never needs the repair there)
    c = cd.scenario_batch(cd.WITNESS_M, chunk=cd.FORCED_CHUNK)
    b = c.names.index("fix_start_0")
    _, sid, st, en = cd.columns(_oracle(oracle, c), c.chars[b, :c.lens[b]], c.M)
    assert cd.repair_items(sid, st, en, int(c.lens[b]), cd.FORCED_CHUNK) == list(range(chunks))      # s at row 0, taken back in the last chunk: every chunk


def _defs(case):
    return [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs, _ in case.defs_t]


def check_host(oracle, case, max_spans):
    """witness_batch_host, match_batch_host and match_batch_host_ragged of a host-only context against the oracle"""
    M = case.M
    cfg = hra.RegexVerifyConfig.configure(M, _defs(case), device=hra.HRX_DEVICE_NONE)
    orec, omsk, ost = _oracle(oracle, case).witness_batch(case.chars, case.lens, M, threads=THREADS)
    ok = (ost & np.uint64(0xff)) == 0
    rec, msk, st = cfg.witness_batch_host(case.chars, case.lens)
    assert np.array_equal(st, ost)
    assert np.array_equal(rec[ok], orec[ok]) and np.array_equal(msk[ok], omsk[ok])
    ecnt, eruns = rle_masked(omsk, case.lens, ost)
    assert max(ecnt) > max_spans
    strings = [bytes(case.chars[b, :case.lens[b]]) for b in range(case.B)]
    for got in (cfg.match_batch_host(case.chars, case.lens, max_spans=max_spans), cfg.match_batch_host_ragged(*hra.pack_strings(strings), max_spans=max_spans)):
        st, cnt, sp = got
        assert np.array_equal(st, ost) and cnt.tolist() == ecnt
        dec = hra.decode_spans(cnt, sp)
        assert all(dec[b] == eruns[b][:max_spans] for b in range(case.B))


@pytest.mark.parametrize("form", sorted(cd.FORMS), ids=sorted(cd.FORMS))
def test_host_walk_on_the_scenarios(oracle, form):
    check_host(oracle, cd.scenario_batch(cd.WITNESS_M, chunk=cd.FORCED_CHUNK, cap=4, **cd.FORMS[form]), 4)


def test_host_walk_on_the_other_batches(oracle):
    check_host(oracle, cd.scenario_batch(8192, chunk=1024, D=2), 4)
    check_host(oracle, cd.all_repair_batch(cd.WITNESS_M, 100, D=3), 2)
    check_host(oracle, cd.block_border_batch(320), 4)


@pytest.mark.parametrize("form", ["one", "second", "three", "big"])
def test_lane_simulation_on_the_scenarios(oracle, sim, form):
    """the tile algebra of csrc/hrx_lane.h re-enacted on the CPU, at the 64-, 32- and 16-row tile words, fix-ups counted"""
    case = cd.scenario_batch(cd.WITNESS_M, chunk=cd.FORCED_CHUNK, **cd.FORMS[form])
    orec, omsk, ost = _oracle(oracle, case).witness_batch(case.chars, case.lens, case.M, threads=THREADS)
    ok = (ost & np.uint64(0xff)) == 0
    s = SimDefs(sim, [(a.encode(), [t.encode() for t in subs]) for a, subs, _ in case.defs_t])
    for W in (64, 32, 16):
        rec, msk, st, fix = s.run(case.chars, case.lens, case.M, W)
        assert np.array_equal(st, ost), W
        assert np.array_equal(rec[ok], orec[ok]) and np.array_equal(msk[ok], omsk[ok]), W
        assert fix > 100, (W, fix)
