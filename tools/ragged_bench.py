"""Ragged input (include/hrx.h RAGGED) against the padded form of the same strings, same process: HIP events around a captured graph of K launches
of one kind, the kinds taking turns.  Per length mix: hrx_match_batch_device_ragged against hrx_match_batch_device on the padded batch (string-major,
and position-major as the headline feeds it); then hrx_ragged_to_position_major_device against hrx_chars_to_position_major_device on full-length
strings.  The ragged and padded results are compared after the timed region.  One JSON line per mix.

  python tools/ragged_bench.py [--config regex1|regex23|headers3] [--mixes all_M,uniform,skewed] [--B 65536] [--M 1024] [--steps 20]
  (with HRX_DEBUG_FLAGS=0x40000 / 0x400000 in the environment: the global-table / HALF form of both kernels)
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/ragged_bench.py      (a run of its own)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import halo2_regex_amd as hra  # noqa: E402
from halo2_regex_amd import synth  # noqa: E402
from oracle_lib import DFA_DIR  # noqa: E402

HDR = lambda n, ns: [n + "_lookup.txt", ["%s_substr%d.txt" % (n, k) for k in range(ns)]]
# config: (defs, generator of planted strings) — one, two and three defs, so D = 1, 2, 3 of both fused kernels
CONFIGS = {"regex1": ([["regex1_test_lookup.txt", ["substr1_test_lookup.txt"]]], synth.regex1_planted),
           "regex23": ([["regex2_test_lookup.txt", ["substr2_test_lookup.txt"]], ["regex3_test_lookup.txt", ["substr3_test_lookup.txt"]]], synth.regex23_planted),
           "headers3": ([HDR("header_from", 1), HDR("header_to", 1), HDR("header_subject", 3)], synth.headers_planted)}


def lengths(mix, B, M, rng):
    if mix == "all_M":
        return np.full(B, M, np.uint32)
    if mix == "uniform":
        return rng.integers(0, M + 1, B).astype(np.uint32)
    if mix == "skewed":          # most strings short, 3 % at M
        lens = rng.integers(0, M // 16, B).astype(np.uint32)
        lens[rng.random(B) < 0.03] = M
        return lens
    raise ValueError(mix)


def timed(kinds, steps, K, dev):
    """kinds: name -> fn(i).  Per launch: the mean over a captured graph of K launches between two events; the kinds alternate."""
    graphs = {}
    s = torch.cuda.Stream(dev)
    for name, fn in kinds.items():
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            fn(0)                   # (first use outside the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(K):
                fn(i)
        graphs[name] = g
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    acc = {k: [] for k in kinds}
    names = list(kinds)
    for i in range(steps):
        for name in (names if i % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); graphs[name].replay(); b.record()
            b.synchronize()
            acc[name].append(a.elapsed_time(b) * 1e3 / K)
    return {k: float(np.median(v)) for k, v in acc.items()}


def one_mix(mix, args, cfg, dev):
    B, M, KS = args.B, args.M, args.max_spans
    rng = np.random.default_rng(0)
    chars, _ = CONFIGS[args.config][1](B, M, seed=0, stride=M)
    lens = lengths(mix, B, M, rng)
    chars[np.arange(M)[None, :] >= lens.astype(np.int64)[:, None]] = 0
    values, offsets = hra.pack_strings([chars[b, :lens[b]].tobytes() for b in range(B)])
    d_vals, d_offs = torch.from_numpy(values).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_chars, d_lens = torch.from_numpy(chars).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
    chars_pm = cfg.chars_to_position_major_device(d_chars)
    outs = {k: (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                torch.empty((B, KS), dtype=torch.int64, device=dev)) for k in ("ragged", "padded_sm", "padded_pm")}
    kinds = {"ragged": lambda i: cfg.match_batch_ragged(d_vals, d_offs, max_spans=KS, out=outs["ragged"]),
             "padded_sm": lambda i: cfg.match_batch(d_chars, d_lens, max_spans=KS, out=outs["padded_sm"]),
             "padded_pm": lambda i: cfg.match_batch(chars_pm, d_lens, max_spans=KS, chars_pm_stride=M, out=outs["padded_pm"])}
    t = timed(kinds, args.steps, args.graph_launches, dev)
    res = {k: [x.cpu().numpy() for x in v] for k, v in outs.items()}
    same = all(np.array_equal(res["ragged"][j], res[k][j]) for k in ("padded_sm", "padded_pm") for j in (0, 1)) and \
        hra.decode_spans(res["ragged"][1].view(np.uint32), res["ragged"][2].view(np.uint64)) == \
        hra.decode_spans(res["padded_pm"][1].view(np.uint32), res["padded_pm"][2].view(np.uint64))
    out = {"config": args.config, "mix": mix, "B": B, "M": M, "mean_len": float(lens.mean()), "values_bytes": int(offsets[-1]),
           "ragged": cfg.describe_match(B, layout=hra.LAYOUT_INPUT_RAGGED), "padded": cfg.describe_match(B, layout=hra.LAYOUT_INPUT_POSITION_MAJOR),
           "ragged_us": t["ragged"], "padded_sm_us": t["padded_sm"], "padded_pm_us": t["padded_pm"],
           "ratio_vs_padded_sm": t["ragged"] / t["padded_sm"], "ratio_vs_padded_pm": t["ragged"] / t["padded_pm"], "same_results": bool(same)}
    if mix == "all_M":       # staging on full-length strings
        stride = -(-M // 16) * 16
        pm_a = torch.empty(B * stride, dtype=torch.uint8, device=dev)
        pm_b = torch.empty(B * stride, dtype=torch.uint8, device=dev)
        l_b = torch.empty(B, dtype=torch.int32, device=dev)
        ts = timed({"ragged_to_pm": lambda i: cfg.ragged_to_position_major(d_vals, d_offs, stride=stride, out=(pm_b, l_b)),
                    "chars_to_pm": lambda i: cfg.chars_to_position_major_device(d_chars, out=pm_a)}, args.steps, args.graph_launches, dev)
        out.update({"ragged_to_pm_us": ts["ragged_to_pm"], "chars_to_pm_us": ts["chars_to_pm"], "staging_ratio": ts["ragged_to_pm"] / ts["chars_to_pm"],
                    "staging_same": bool(torch.equal(pm_a, pm_b) and torch.equal(l_b, d_lens))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="regex1", choices=list(CONFIGS))
    ap.add_argument("--mixes", default="all_M,uniform,skewed")
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--max-spans", type=int, default=16)
    ap.add_argument("--graph-launches", type=int, default=10, help="launches per captured graph (one timed interval)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    defs = [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(os.path.join(DFA_DIR, a)), [hra.SubstrRegexDef.read_from_text(os.path.join(DFA_DIR, s)) for s in subs])
            for a, subs in CONFIGS[args.config][0]]
    cfg = hra.RegexVerifyConfig.configure(args.M, defs, device=0)
    for mix in args.mixes.split(","):
        print(json.dumps(one_mix(mix, args, cfg, dev)), flush=True)


if __name__ == "__main__":
    main()
