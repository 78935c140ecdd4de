"""The launch planner against a recorded net: tests/golden/launch_plans.json holds what hrx_describe_launch / hrx_describe_match answered, over the sweep of
tests/golden/record_launch_plans.py, in a library built from the commit named in the fixture — before the planner moved into csrc/hrx_plan.cpp and launch and
describe came to read one route plan.  The built library must answer every line of the sweep with the same texts: a threshold that moves by one group, a
ring one slot shallower, another kernel for one shape all change a line's digest.  Where the parent's text disagreed with the parent's own launch, the
fixture keeps the parent's line and a NOTE beside it (record_launch_plans.NOTES): the corrected digest, and a rule that the difference must satisfy.
No device is needed: the planner is host code."""
import importlib.util
import os
import re

import pytest

import halo2_regex_amd as hra
from oracle_lib import ROOT

_spec = importlib.util.spec_from_file_location("record_launch_plans", os.path.join(ROOT, "tests", "golden", "record_launch_plans.py"))
rlp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rlp)

LARGEST_FIXTURE = 441818        # bytes of tests/golden/compiler/cases.json: no fixture is larger

# every form the planner can return, as it shows in a text; each must rest on at least MIN_LINES lines of the fixture's own sample texts
MIN_LINES = 3
PM = r"witness_pm_kernel<\d, %s>"
FORMS = {
    "pair-step kernel": r"hrx::witness_pp_kernel ",
    "def-parallel, WIDE": r"witness_pmd_kernel<\d+, false, false, false>",
    "def-parallel, WIDE, combiner wave": r"witness_pmd_kernel<\d+, false, true, false>",
    "def-parallel, CLASS-WIDE": r"witness_pmd_kernel<\d+, true, true, false>",
    "def-parallel, CLASS-WIDE, string-major": r"witness_pmd_kernel<\d+, true, true, true> .* sub-tiles=\d",
    "loader/walker, global table": PM % r"true, \w+, \w+, \w+, \w+",
    "loader/walker, WIDE": PM % r"\w+, true, \w+, \w+, \w+",
    "loader/walker, HALF": PM % r"\w+, \w+, true, \w+, \w+",
    "loader/walker, string-major": PM % r"\w+, \w+, \w+, true, \w+",
    "loader/walker, BYTE": PM % r"\w+, \w+, \w+, \w+, true",
    "walker/storer, 4-byte": r"witness_split_kernel<\d, \d+, false>",
    "walker/storer, BYTE": r"witness_split_kernel<1, 32, true>",
    "one-wave, 64 strings": r"witness_kernel<.* gs=64",
    "one-wave, 32 strings": r"witness_kernel<.* gs=32",
    "one-wave, 16 strings": r"witness_kernel<.* gs=16",
    "chunked": r" chunked=\d+x\d+ tiles",
    "dynamic groups": r" groups=dynamic",
    "multi-pass, merged by the last pass": r"^multi-pass, .*\(the last pass merges the summaries\) \+ hrx::witness_merge_status_kernel",
    "multi-pass, summary combine": r"^multi-pass, .*\+ hrx::witness_combine_summary_kernel",
    "multi-pass, copy-mode combine": r"^multi-pass, .*\+ hrx::witness_combine_kernel<true>",
    "transpose": r" \+ hrx::transpose_pm_to_sm_kernel$",
    "match, fused, padded": r"^hrx::match_lane_kernel<",
    "match, fused, ragged": r"^hrx::match_ragged_kernel<",
    "match, fused, selected": r"^hrx::match_selected_kernel<",
    "match, via rows, padded": r"^via rows, \d+ slice\(s\) of \d+ strings: (hrx::pm_input_slice_kernel \+ )?(hrx::witness|multi-pass)",
    "match, via rows, ragged": r"^via rows, .*: hrx::ragged_slice_kernel \+ ",
    "match, via rows, selected": r"^via rows, .*: hrx::selected_slice_kernel<hrx::\w+> \+ .* \+ hrx::spans_from_masked_selected_kernel$",
    "no launch fits": r"^ERR %d: " % hra.HRX_ERR_BOUNDS,
}


@pytest.fixture(scope="module")
def fixture():
    return rlp.load_fixture()


def test_fixture_is_the_parents_and_small(fixture):
    assert re.fullmatch(r"[0-9a-f]{40}", fixture["recorded_from_commit"])
    assert os.path.getsize(rlp.FIXTURE) < LARGEST_FIXTURE
    lines = rlp.sweep()
    assert fixture["lines"] == len(lines) == len(fixture["digests"]) == len(fixture["samples"])
    assert all(len(refs) == len(rlp.samples(line[4])) for line, refs in zip(lines, fixture["samples"]))
    # notes: every one names a rule of the recorder and says why; a noted line keeps the parent's digest beside the corrected one
    assert set(fixture.get("notes", {})) <= set(rlp.NOTES) and all(len(n["reason"]) > 80 for n in fixture.get("notes", {}).values())
    assert all(d != fixture["digests"][i] for i, (_, d) in fixture["noted"].items()) and len(fixture["noted"]) < len(lines) // 10


def test_the_sweep_names_every_form_the_planner_returns(fixture):
    texts, counts = fixture["texts"], {}
    hit = {name: [i for i, t in enumerate(texts) if re.search(pat, t)] for name, pat in FORMS.items()}
    for name, idx in hit.items():
        idx = set(idx)
        counts[name] = sum(1 for refs in fixture["samples"] if idx.intersection(refs))
    thin = {name: n for name, n in counts.items() if n < MIN_LINES}
    assert not thin, thin
    # an answer that is an error is recorded as one, with the library's message
    assert any(t.startswith("ERR %d: " % hra.HRX_ERR_BOUNDS) and "do not fit" in t for t in texts)
    assert not [t for t in texts if t.startswith("ERR ") and not t.startswith("ERR %d: " % hra.HRX_ERR_BOUNDS)]


def test_built_library_plans_what_the_parent_planned(fixture):
    texts, bad = fixture["texts"], []

    def check(i, line, bs, got):
        want = {B: texts[r] for B, r in zip(rlp.samples(line[4]), fixture["samples"][i])}
        ok = rlp.digest(got) == fixture["digests"][i]
        if not ok and i in fixture["noted"]:      # a line whose parent text disagreed with the parent's launch: the corrected text, and only the noted difference
            name, d = fixture["noted"][i]
            ok = rlp.digest(got) == d and all(t == want[B] or rlp.NOTES[name][1](want[B], t) for B, t in zip(bs, got) if B in want)
        if not ok:
            bad.append((rlp.key_of(line), [(B, t, want.get(B)) for B, t in zip(bs, got)]))
    rlp.run_sweep(hra, check)
    for key, rows in bad[:8]:
        print("MISMATCH %s" % key)
        for B, got, want in rows:
            print("    B=%d got:  %s" % (B, got))
            if want is not None and want != got:
                print("    B=%d want: %s" % (B, want))
    assert not bad, "%d line(s) differ from the plans of %s (first: %s); record_launch_plans.py --dump shows every text" % (
        len(bad), fixture["recorded_from_commit"][:12], bad[0][0])


def test_scout_tables_under_asan_and_ubsan(tmp_path):
    """tests/host_cpp/test_scout_tables.cpp: build_scout_tables (csrc/hrx_defs.cpp, the tables of the chunked launch's scout) as a program of its own under the
    address and undefined-behaviour sanitizers: compact image and quasi-absorbing bits of three small def sets against the narrow table, entry by entry"""
    import subprocess
    exe = str(tmp_path / "hrx_test_scout_tables")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cpp", "test_scout_tables.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "scout tables: ok" in out.stdout, out.stdout + out.stderr
