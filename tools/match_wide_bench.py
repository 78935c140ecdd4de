#!/usr/bin/env python3
"""Fused-wide match against via rows on one device (HRX_OPT_MATCH_FUSED_WIDE): the four header defs + regex1 (--double: the set twice
over, eight defs) on synth.headers_planted, B = 65536 x M = 1024 (and 4 x 65536 uniform with --big), the three length mixes of tools/ragged_bench.py, ragged
and string-major input, and the cascade of DESIGN.md §15 item 4 (every third string ends in what regex1 accepts; the survivors of a regex1 screen go through
match_selected).

Method: every kind is captured as a graph of 10 launches on one stream; the kinds take turns in one process, 20 rounds, medians.  The yardstick of every
line is the via-rows launch of the same config with the option at 0, timed twice (the two figures' difference is the noise floor); the ratio is against the
smaller.  Every fused-wide result is compared with the via-rows result (a cascade's at the selected indices) before anything is timed.

MI355X, 2026-10-19, one lease, us per launch, fused wide / via rows (its two figures) = ratio:
  four defs   all n = M   ragged 233.2 / 555.9 555.7 = 0.42   string-major 234.7 / 513.8 513.6 = 0.46   cascade (21846 of 65536)  232.0 / 238.4 238.2 = 0.97
              uniform     ragged 616.8 / 659.3 655.5 = 0.94   string-major 619.5 / 637.7 635.2 = 0.98   cascade (21315)           631.0 / 294.1 290.7 = 2.17
              skewed      ragged 517.8 / 656.0 646.2 = 0.80   string-major 518.0 / 633.0 624.1 = 0.83   cascade (13520)           520.6 / 202.2 200.6 = 2.60
              4 x 65536 uniform (sweeps of one def)   ragged 1715.1 / 2461.8 2457.9 = 0.70   string-major 1727.8 / 2320.4 2318.0 = 0.75   cascade (85275) 883.1 / 964.2 957.9 = 0.92
  eight defs  all n = M   ragged 425.0 / 709.8 709.8 = 0.60   string-major 424.6 / 708.3 708.5 = 0.60   cascade 426.0 / 253.5 252.0 = 1.69
              uniform     ragged 1133.4 / 1048.4 1051.5 = 1.08   string-major 1136.7 / 1005.5 1006.3 = 1.13   cascade 1156.8 / 301.0 301.9 = 3.84
              skewed      ragged 923.7 / 1067.9 1071.9 = 0.87   string-major 923.8 / 1034.9 1033.0 = 0.89   cascade 920.2 / 142.3 144.7 = 6.47
These figures were taken with a build that also instantiated sweeps of one and two defs for every def count (the G sweep: NOTES_MEASUREMENTS.md §16 has
its raw lines); the library keeps the widths that sweep chose."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_regex_amd as hra  # noqa: E402
from halo2_regex_amd import synth  # noqa: E402

DFA = os.path.join(ROOT, "tests", "golden", "dfa")
HDR = lambda n, ns: [n + "_lookup.txt", ["%s_substr%d.txt" % (n, k) for k in range(ns)]]
CFG_1 = [["regex1_test_lookup.txt", ["substr1_test_lookup.txt"]]]
CFG_H4 = [HDR("header_from", 1), HDR("header_to", 1), HDR("header_subject", 3)] + CFG_1
OPT = hra.OPT_MATCH_FUSED_WIDE
DEV = torch.device("cuda", 0)


def config(names, M, wide):
    defs = [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(os.path.join(DFA, a)), [hra.SubstrRegexDef.read_from_text(os.path.join(DFA, s)) for s in subs])
            for a, subs in names]
    cfg = hra.RegexVerifyConfig.configure(M, defs, device=0)
    cfg.set_option(OPT, wide)
    return cfg


def lengths(kind, B, M, rng):
    if kind == "all_M":
        return np.full(B, M, np.uint32)
    if kind == "uniform":
        return rng.integers(0, M + 1, B).astype(np.uint32)
    lens = rng.integers(0, max(2, M // 16), B).astype(np.uint32)      # skewed: most strings short, a few at M
    lens[rng.random(B) < 0.03] = M
    return lens


def column(chars, lens):
    L = lens.astype(np.int64)
    offsets = np.zeros(len(L) + 1, np.int64)
    np.cumsum(L, out=offsets[1:])
    values = np.zeros(-(-int(offsets[-1]) // 16) * 16 + 16, np.uint8)
    values[:int(offsets[-1])] = chars[np.arange(chars.shape[1])[None, :] < L[:, None]]
    return values, offsets


def time_kinds(kinds, rounds=20, launches=10):
    """kinds: name -> fn(stream); -> name -> median microseconds per launch.  One stream for every graph, each kind's first use on it and outside the capture
    (the via-rows scratch is allocated at first use and belongs to one stream at a time), graphs of `launches` launches, the kinds taking turns"""
    s = torch.cuda.Stream(DEV)
    graphs = {}
    for name, fn in kinds.items():
        s.wait_stream(torch.cuda.current_stream(DEV))
        fn(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(launches):
                fn(s)
        graphs[name] = g
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(rounds):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                a.record()
                g.replay()
                b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1000.0 / launches)
    return {k: statistics.median(v) for k, v in times.items()}


def same(a, b, idx=None):
    """status, counts and runs of two calls equal (idx: at these string indices only — a selected call touches no other entry)"""
    torch.cuda.synchronize()
    st, cnt, sp = (t.cpu().numpy() for t in a)
    st2, cnt2, sp2 = (t.cpu().numpy() for t in b)
    if idx is not None:
        st, cnt, sp, st2, cnt2, sp2 = (x[idx] for x in (st, cnt, sp, st2, cnt2, sp2))
    return np.array_equal(st, st2) and np.array_equal(cnt, cnt2) and hra.decode_spans(cnt.view(np.uint32), sp.view(np.uint64)) == hra.decode_spans(cnt2.view(np.uint32), sp2.view(np.uint64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--big", action="store_true", help="also B x 4, uniform lengths, one run")
    ap.add_argument("--double", action="store_true", help="the def set twice over (eight defs) instead of four")
    args = ap.parse_args()
    M = args.M
    names = CFG_H4 * 2 if args.double else CFG_H4
    wides = {"fused wide": config(names, M, 1)}
    off, screen = config(names, M, 0), config(CFG_1, M, 0)
    for name, cfg in wides.items():
        print("%s: %s" % (name, cfg.describe_match(args.B, layout=hra.LAYOUT_INPUT_RAGGED)))
    shapes = [(args.B, k) for k in ("all_M", "uniform", "skewed")] + ([(4 * args.B, "uniform")] if args.big else [])
    for B, mix in shapes:
        rng = np.random.default_rng(1)
        chars, _ = synth.headers_planted(B, M, seed=3, stride=M + 16)
        lens = lengths(mix, B, M, rng)
        hit = np.frombuffer(b"email was meant for @bob.", np.uint8)       # every third string ends in what regex1 accepts: the cascade's survivors
        for b in range(0, B, 3):
            if lens[b] >= len(hit):
                chars[b, int(lens[b]) - len(hit):int(lens[b])] = hit
        chars[np.arange(chars.shape[1])[None, :] >= lens.astype(np.int64)[:, None]] = 0
        values, offsets = column(chars, lens)
        d_chars, d_lens = torch.from_numpy(chars).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV)
        d_vals, d_offs = torch.from_numpy(values).to(DEV), torch.from_numpy(offsets).to(DEV)
        st1 = screen.match_batch(d_chars, d_lens)[0]
        r = screen.route(st1, lens=d_lens, bounds=[M], require_accept=1)
        d_sel = r.order[:int(r.bucket_offsets.cpu()[1])].contiguous()
        idx = d_sel.cpu().numpy().view(np.uint32).astype(np.int64)
        outs = {}

        def call(cfg, form, key):
            def fn(stream):
                if form == "ragged":
                    outs[key] = cfg.match_batch_ragged(d_vals, d_offs, out=outs.get(key), stream=stream)
                elif form == "string_major":
                    outs[key] = cfg.match_batch(d_chars, d_lens, out=outs.get(key), stream=stream)
                else:
                    outs[key] = cfg.match_selected(d_chars, d_sel, lens=d_lens, out=outs.get(key), stream=stream)
            return fn

        for form in ("ragged", "string_major", "cascade"):
            if form == "cascade" and d_sel.numel() == 0:
                continue
            fns = {name: call(cfg, form, form + name) for name, cfg in wides.items()}
            fns["via rows"] = fns["via rows again"] = call(off, form, form + "v")
            s0 = torch.cuda.current_stream(DEV)
            for name, fn in fns.items():
                fn(s0)
            torch.cuda.synchronize()        # (the timing's stream takes the via-rows scratch over from here: a host wait, outside any capture)
            for name in wides:
                if not same(outs[form + name], outs[form + "v"], idx if form == "cascade" else None):
                    print("%s %s %s: RESULTS DIFFER" % (mix, form, name))
                    return 1
            t = time_kinds(fns)
            via = min(t["via rows"], t["via rows again"])
            print("B=%d %-8s %-12s n=%-6d via rows %8.1f / %8.1f us  " % (B, mix, form, d_sel.numel() if form == "cascade" else B, t["via rows"], t["via rows again"]) +
                  "  ".join("%s %8.1f us ratio %.3f" % (name, t[name], t[name] / via) for name in wides), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
