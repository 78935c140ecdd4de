#!/usr/bin/env python3
"""LOOKUP COUNTS: hrx_lookup_counts_device on regex1 at 65536 x 1024, regex2 + regex3 at 65536 x 2048 and regex1 at 8192 x 32768 (in windows of
2048 strings: one call per window, the figure is their sum), position-major interleaved records, position-major input.

Method: a graph of `--launches` calls per shape on one stream, `--rounds` replays, the median, us per call.  Before anything is timed the device counts and
misses of the whole shape must equal the host twin's (hrx_lookup_counts_host on the rows copied out, HRX_OPT_HOST_THREADS = 16), word for word; the tool stops
otherwise.  The host twin's wall time on the same input is the second figure.

There is no earlier implementation to compare with, so the only yardsticks are a byte count and the host twin: the algorithmic bytes of a call are
rows x (1 + 4 D) read plus b_count x W x 4 written, and the tool prints what fraction of 8 TB/s they amount to at the measured time.  --json FILE: the figures
as a JSON list (profiles/lookup_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_regex_amd as hra  # noqa: E402
from halo2_regex_amd import synth  # noqa: E402

DFA = os.path.join(ROOT, "tests", "golden", "dfa")
CFG_1 = [["regex1_test_lookup.txt", ["substr1_test_lookup.txt"]]]
CFG_23 = [["regex2_test_lookup.txt", ["substr2_test_lookup.txt"]], ["regex3_test_lookup.txt", ["substr3_test_lookup.txt"]]]
DEV = torch.device("cuda", 0)
PM_IN = hra.LAYOUT_POSITION_MAJOR | hra.LAYOUT_INPUT_POSITION_MAJOR
PEAK = 8e12                   # bytes per second


def config(names, M):
    defs = [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(os.path.join(DFA, a)), [hra.SubstrRegexDef.read_from_text(os.path.join(DFA, s)) for s in subs])
            for a, subs in names]
    return hra.RegexVerifyConfig.configure(M, defs, device=0)


def time_graph(fn, rounds, launches):
    """fn(stream) -> median microseconds per call"""
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    fn(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(launches):
            fn(s)
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            a.record()
            g.replay()
            b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0 / launches)
    return statistics.median(times)


def run_shape(label, names, B, M, make, window, rounds, launches):
    cfg = config(names, M)
    cfg.set_option(hra.OPT_HOST_THREADS, 16)
    D, W = cfg.num_defs, cfg.lookup_words()
    chars, lens = make(B, M - 8, stride=M + 16)
    stride = chars.shape[1]
    d_pm = hra.chars_to_position_major(torch.from_numpy(chars).to(DEV))
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    out = cfg.witness_batch_position_major(d_pm, d_lens, chars_pm_stride=stride)
    window = min(window or B, B)
    counts = torch.empty((B, W), dtype=torch.int32, device=DEV)
    misses = torch.empty((B,), dtype=torch.int32, device=DEV)

    def device(s):
        for b0 in range(0, B, window):
            n = min(window, B - b0)
            cfg.lookup_counts(d_pm, d_lens, out[0], layout=PM_IN, b_begin=b0, b_count=n, out=counts[b0:b0 + n], misses=misses[b0:b0 + n], chars_pm_stride=stride, stream=s)

    device(torch.cuda.current_stream(DEV))
    torch.cuda.synchronize()
    h_chars, h_rec = d_pm.cpu().numpy(), out[0].cpu().numpy().view(np.uint32)
    h_counts, h_misses = np.empty((B, W), np.uint32), np.empty(B, np.uint32)
    cfg.lookup_counts_host(h_chars, lens, h_rec, layout=PM_IN, out=h_counts, misses=h_misses, chars_pm_stride=stride)      # (the first call builds the image)
    t0 = time.perf_counter()
    cfg.lookup_counts_host(h_chars, lens, h_rec, layout=PM_IN, out=h_counts, misses=h_misses, chars_pm_stride=stride)
    host_ms = (time.perf_counter() - t0) * 1e3
    if not (np.array_equal(counts.cpu().numpy().view(np.uint32), h_counts) and np.array_equal(misses.cpu().numpy().view(np.uint32), h_misses)):
        print("%s: the device counts differ from the host twin's" % label)
        return None
    us = time_graph(device, rounds, launches)
    read, written = B * M * (1 + 4 * D), B * W * 4
    group, passes = cfg.lookup_group(window)
    res = {"shape": label, "B": B, "M": M, "D": D, "W": W, "window": window, "calls": -(-B // window), "group": group, "passes": passes, "device_us": round(us, 1),
           "bytes_read": read, "bytes_written": written, "fraction_of_8TBps": round((read + written) / (us * 1e-6) / PEAK, 4), "host_twin_16_threads_ms": round(host_ms, 1),
           "strings_with_misses": int((h_misses != 0).sum())}
    print("%-26s B=%d M=%d D=%d W=%d  window %d (G=%d)  device %9.1f us  = %.3f of 8 TB/s over %.0f MB read + %.0f MB written   host twin, 16 threads %8.1f ms (%.0f times)"
          % (label, B, M, D, W, window, group, us, res["fraction_of_8TBps"], read / 1e6, written / 1e6, host_ms, host_ms * 1e3 / us), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    shapes = [("regex1", CFG_1, args.B, 1024, synth.regex1_planted, 0), ("regex2 + regex3", CFG_23, args.B, 2048, synth.regex23_planted, 0)]
    if not args.skip_long:
        shapes.append(("regex1 long, windowed", CFG_1, args.B // 8, 32768, synth.regex1_planted, 2048))
    results = []
    for label, names, B, M, make, window in shapes:
        r = run_shape(label, names, B, M, make, window, args.rounds, args.launches)
        if r is None:
            return 1
        results.append(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
