"""Match launch (hrx_match_batch_device) against the witness launch (hrx_witness_batch_device_layout, position-major) on the same batch, same process:
HIP events around a captured graph of K launches of one kind over rotating output sets, the two kinds alternating; then hrx_match_batch_host against hrx_witness_batch_host on the headline batch.  Every string's
status and runs are checked against the oracle after the timed region.  One JSON line per shape.

  python tools/match_bench.py [--shapes regex1,regex23,...] [--steps 20] [--warmup 5]
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/match_bench.py --shapes regex1 --no-host   (a run of its own)
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

import bench  # noqa: E402  (workload(): the bench's own batches)
import halo2_regex_amd as hra  # noqa: E402
from oracle_lib import OracleDefs, load_oracle  # noqa: E402

# name: (bench config, B, M)
SHAPES = {"regex1": ("regex1", 65536, 1024), "regex23": ("regex23", 262144, 2048), "headers3": ("headers3", 32768, 32768),
          "dfa256": ("dfa256", 131072, 4096), "headers4": ("headers4", 65536, 2048), "regex1_long": ("regex1", 8192, 32768)}


def one_shape(name, args, dev):
    cfgname, B, M = SHAPES[name]
    ns = argparse.Namespace(config=cfgname, dist="planted", substr_defs=1, substr_pairs=40)
    names, label, _, gen, _ = bench.workload(ns)
    defs = [hra.RegexDefs(hra.AllstrRegexDef(a.decode()), [hra.SubstrRegexDef(s.decode()) for s in subs]) for a, subs in names]
    cfg = hra.RegexVerifyConfig.configure(M, defs, device=0)
    chars, lens = gen(B, M - 1, seed=0, stride=M)
    d_chars = torch.from_numpy(chars).to(dev)
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(dev)
    chars_pm = hra.chars_to_position_major(d_chars)
    KS = args.max_spans
    nset = 2
    msets = [(torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, max(KS, 1)), dtype=torch.int64, device=dev))
             for _ in range(nset)]
    wsets = [cfg.alloc_outputs_position_major(B, dev) for _ in range(nset)]
    match = lambda i: cfg.match_batch(chars_pm, d_lens, max_spans=KS, chars_pm_stride=M, out=msets[i % nset])
    witness = lambda i: cfg.witness_batch_position_major(chars_pm, d_lens, out=wsets[i % nset], chars_pm_stride=M)
    for i in range(args.warmup):
        match(i); witness(i)
    torch.cuda.synchronize()
    # per launch: the mean over K launches of one kind between two events, as bench.py times its K steps — a captured graph of them where the launch can
    # be captured (no host submission inside the timed interval), else K launches queued back to back; the two kinds alternate
    K = args.graph_launches
    fused = cfg.describe_match(B, layout=hra.LAYOUT_INPUT_POSITION_MAJOR).startswith("hrx::match_lane_kernel")
    runs = {}
    s = torch.cuda.Stream(dev)
    for kind, fn in (("match", match), ("witness", witness)):
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            fn(0)                                       # (first use outside a capture: scratch, LDS attributes)
        torch.cuda.synchronize()
        try:
            if not fused:      # ("via rows" shapes: their witness launches may need host waits, which a capture does not allow)
                raise RuntimeError("not captured")
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                for i in range(K):
                    fn(i)
            runs[kind] = ("graph", g.replay)
        except Exception:
            torch.cuda.synchronize()
            runs[kind] = ("eager", lambda fn=fn: [fn(i) for i in range(K)])
    for _ in range(2):
        runs["match"][1](); runs["witness"][1]()
    torch.cuda.synchronize()
    tm, tw = [], []
    for i in range(args.steps):
        for kind, acc in (("match", tm), ("witness", tw)) if i % 2 == 0 else (("witness", tw), ("match", tm)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); runs[kind][1](); b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b) * 1e3 / K)
    out = {"shape": name, "label": label, "B": B, "M": M, "match": cfg.describe_match(B, layout=hra.LAYOUT_INPUT_POSITION_MAJOR),
           "match_us_median": float(np.median(tm)), "witness_us_median": float(np.median(tw)), "match_us_min": float(min(tm)), "witness_us_min": float(min(tw)),
           "timing": {k: v[0] for k, v in runs.items()}, "launches_per_interval": K}
    out["speedup"] = out["witness_us_median"] / out["match_us_median"]
    if not args.no_verify:      # after the timed region
        st, cnt, sp = (t.cpu().numpy() for t in msets[(args.steps - 1) % nset])
        _, omsk, ost = OracleDefs(load_oracle(), names).witness_batch(chars, lens, M, threads=16)
        ecnt, eruns = hra.runs_from_masked(omsk, lens, ost)
        dec = hra.decode_spans(cnt.view(np.uint32), sp.view(np.uint64))
        out["verified"] = bool(np.array_equal(st.view(np.uint64), ost) and cnt.view(np.uint32).tolist() == ecnt and
                               all(dec[b] == eruns[b][:KS] for b in range(B)))
    if name == "regex1" and not args.no_host:
        th, tw2 = [], []
        for i in range(max(3, args.steps // 4)):
            t0 = time.perf_counter(); cfg.match_batch_host(chars, lens, max_spans=KS); th.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); cfg.witness_batch_host(chars, lens); tw2.append((time.perf_counter() - t0) * 1e3)
        out["match_host_ms_median"], out["witness_host_ms_median"] = float(np.median(th)), float(np.median(tw2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-spans", type=int, default=16)
    ap.add_argument("--graph-launches", type=int, default=10, help="launches per captured graph (one timed interval)")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.shapes.split(","):
        print(json.dumps(one_shape(name, args, dev)), flush=True)


if __name__ == "__main__":
    main()
