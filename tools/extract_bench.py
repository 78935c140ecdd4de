"""EXTRACT (include/hrx.h) against the match launch it follows, same process, the method of tools/ragged_bench.py: HIP events around a captured graph of K
launches of one kind, the kinds taking turns, medians over --steps intervals.  Per case (regex1 planted; reveal_stress on regex1 + regex2, where about a
quarter of the bytes is revealed) and input form (string-major, position-major, ragged): the match launch alone, match + extract in one graph, their
difference (the added step) and its ratio to the match launch; and the host wall time of the route it replaces — revealed_substrings on the same match
outputs, its device-to-host copies included.  Every run checks the extracted column against revealed_substrings.  One JSON line per case and form.

  python tools/extract_bench.py [--cases planted,stress] [--forms sm,pm,ragged] [--B 65536] [--M 1024] [--steps 20]
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/extract_bench.py --steps 2      (a run of its own: the four kernels' times)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import halo2_regex_amd as hra  # noqa: E402
from halo2_regex_amd import synth  # noqa: E402
from oracle_lib import DFA_DIR  # noqa: E402
from ragged_bench import timed  # noqa: E402

R1 = ["regex1_test_lookup.txt", ["substr1_test_lookup.txt"]]
R2 = ["regex2_test_lookup.txt", ["substr2_test_lookup.txt"]]
CASES = {"planted": ([R1], lambda B, M: synth.regex1_planted(B, M - 1, seed=0, stride=M)),
         "stress": ([R1, R2], lambda B, M: synth.reveal_stress(B, M, seed=9))}


def one(case, form, args, dev):
    B, M, K = args.B, args.M, args.max_spans
    names, gen = CASES[case]
    defs = [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(os.path.join(DFA_DIR, a)), [hra.SubstrRegexDef.read_from_text(os.path.join(DFA_DIR, s)) for s in subs])
            for a, subs in names]
    cfg = hra.RegexVerifyConfig.configure(M, defs, device=0)
    chars, lens = gen(B, M)
    chars = np.ascontiguousarray(chars[:, :M]) if chars.shape[1] >= M else np.pad(chars, ((0, 0), (0, M - chars.shape[1])))
    lens = np.minimum(lens, M).astype(np.uint32)
    if form == "ragged":
        values, offsets = hra.pack_strings([chars[b, :lens[b]].tobytes() for b in range(B)])
        src = (torch.from_numpy(values).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev))
        out = cfg.alloc_extract(B, K, len(values))
        match = lambda i: cfg.match_batch_ragged(*src, max_spans=K, out=out[:3])
        both = lambda i: cfg.extract_batch_ragged(*src, max_spans=K, out=out)
        in_bytes = int(offsets[-1])
    else:
        d_chars, d_lens = torch.from_numpy(chars).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
        kw = {}
        if form == "pm":
            d_in, kw = cfg.chars_to_position_major_device(d_chars), {"chars_pm_stride": M}
        else:
            d_in = d_chars
        out = cfg.alloc_extract(B, K, chars.size)
        match = lambda i: cfg.match_batch(d_in, d_lens, max_spans=K, out=out[:3], **kw)
        both = lambda i: cfg.extract_batch(d_in, d_lens, max_spans=K, out=out, **kw)
        in_bytes = chars.size
    t = timed({"match": match, "match_extract": both}, args.steps, args.graph_launches, dev)
    ex = both(0)
    torch.cuda.synchronize()
    # today's route on the same match outputs: the input and the spans come back to the host, a Python loop slices them
    t0 = time.perf_counter()
    if form == "ragged":
        old = hra.revealed_substrings_ragged(src[0], src[1], out[0], out[1], out[2])
    else:
        old = hra.revealed_substrings(d_chars, d_lens, out[0], out[1], out[2])
    t_old = time.perf_counter() - t0
    # ... and the new one end to end on the host side: totals, then only the filled part of the column
    t0 = time.perf_counter()
    tot = ex.totals.cpu().numpy()
    col = (ex.run_offsets.cpu(), ex.runs[:int(tot[0])].cpu(), ex.byte_offsets[:int(tot[0]) + 1].cpu(), ex.values[:int(tot[1])].cpu())
    t_new = time.perf_counter() - t0
    same = hra.extracted_lists(ex) == old
    del col
    added = t["match_extract"] - t["match"]
    return {"case": case, "form": form, "B": B, "M": M, "max_spans": K, "input_bytes": in_bytes, "runs": int(tot[0]), "revealed_bytes": int(tot[1]),
            "truncated_strings": int(tot[2]), "match": cfg.describe_match(B, layout={"sm": 0, "pm": 2, "ragged": 8}[form]),
            "match_us": t["match"], "match_extract_us": t["match_extract"], "extract_us": added, "extract_over_match": added / t["match"],
            "revealed_substrings_host_ms": t_old * 1e3, "column_to_host_ms": t_new * 1e3, "same_as_revealed_substrings": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="planted,stress")
    ap.add_argument("--forms", default="sm,pm,ragged")
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--max-spans", type=int, default=16)
    ap.add_argument("--graph-launches", type=int, default=10, help="launches per captured graph (one timed interval)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for case in args.cases.split(","):
        for form in args.forms.split(","):
            print(json.dumps(one(case, form, args, dev)), flush=True)


if __name__ == "__main__":
    main()
