#!/usr/bin/env python3
"""LOOKUP COMPRESS: hrx_lookup_compress_inputs_device on regex1 at 65536 x 1024, regex2 + regex3 at 65536 x 2048 (in windows of 16384 strings)
and regex1 at 8192 x 32768 (in four windows: one call per window, the figure is their sum), position-major interleaved records, position-major input, one
challenge per string, Montgomery limbs; and hrx_lookup_compress_table_device at 1 and 4096 runs.

Method: a graph of `--launches` calls per shape on one stream, `--rounds` replays, the median, us per call.  Before anything is timed the device cells of the
whole shape must equal the host twin's (hrx_lookup_compress_inputs_host on the rows copied out, HRX_OPT_HOST_THREADS = 16), limb for limb, chunk by chunk;
the tool stops otherwise.

Nobody has measured such a kernel here and no threshold is set.  In the same run, on the same rows, the two yardsticks that exist without it are timed:
hrx_fr_columns_device, as bytes of cells written per second (the same store pattern without a fold), and the host twin's wall time on 16 threads.  Per shape:
us per call; the fraction of 8 TB/s over the algorithmic bytes, rows x (1 + 4 D) read plus 32 x 3 D per row written; the ratio of the cell byte rates; the
ratio to the host twin.  --json FILE: the figures as a JSON list (profiles/compress_bench.json); --label: the name the figures carry, for runs
that compare two libraries through HRX_LIB_PATH."""
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
CHECK_BYTES = 1 << 29         # cells compared per chunk


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


def random_theta(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)


def run_shape(label, variant, names, B, M, make, window, rounds, launches):
    cfg = config(names, M)
    cfg.set_option(hra.OPT_HOST_THREADS, 16)
    D = cfg.num_defs
    chars, lens = make(B, M - 8, stride=M + 16)
    stride = chars.shape[1]
    d_pm = hra.chars_to_position_major(torch.from_numpy(chars).to(DEV))
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    out = cfg.witness_batch_position_major(d_pm, d_lens, chars_pm_stride=stride)
    window = min(window or B, B)
    theta = random_theta(B, 1)
    d_theta = torch.from_numpy(theta.view(np.int64)).to(DEV)
    cells = torch.empty((3 * D, window, M, 4), dtype=torch.int64, device=DEV)        # one window's cells; every window of a call is written here in turn

    def one_window(b0, n, dst, s):
        cfg.lookup_compress_inputs(d_pm, d_lens, out[0], d_theta[b0:b0 + n], layout=PM_IN, b_begin=b0, b_count=n, out=dst, chars_pm_stride=stride, stream=s)

    def device(s):
        for b0 in range(0, B, window):
            n = min(window, B - b0)
            one_window(b0, n, cells.view(-1)[:3 * D * n * M * 4].view(3 * D, n, M, 4), s)

    # the whole shape against the host twin, chunk by chunk
    h_chars, h_rec = d_pm.cpu().numpy(), out[0].cpu().numpy().view(np.uint32)
    chunk = max(1, min(window, CHECK_BYTES // (3 * D * M * 32)))
    h_cells = np.zeros((3 * D, chunk, M, 4), np.uint64)
    host_s = 0.0
    for b0 in range(0, B, chunk):
        n = min(chunk, B - b0)
        dst = cells.view(-1)[:3 * D * n * M * 4].view(3 * D, n, M, 4)
        one_window(b0, n, dst, torch.cuda.current_stream(DEV))
        torch.cuda.synchronize()
        want = h_cells.reshape(-1)[:3 * D * n * M * 4].reshape(3 * D, n, M, 4)
        t0 = time.perf_counter()
        cfg.lookup_compress_inputs_host(h_chars, lens, h_rec, theta[b0:b0 + n], layout=PM_IN, b_begin=b0, b_count=n, out=want, chars_pm_stride=stride)
        host_s += time.perf_counter() - t0
        if not np.array_equal(dst.cpu().numpy().view(np.uint64), want):
            print("%s: the device cells of strings %d .. %d differ from the host twin's" % (label, b0, b0 + n))
            return None
    del h_cells
    us = time_graph(device, rounds, launches)
    rows = B * M
    read, written = rows * (1 + 4 * D), rows * 32 * 3 * D
    # the yardstick: the field cells of the same rows, window by window
    del cells
    ncols = 4 + 4 * D
    fr_cells = torch.empty((ncols, window, M, 4), dtype=torch.int64, device=DEV)

    def fr(s):
        for b0 in range(0, B, window):
            n = min(window, B - b0)
            cfg.fr_columns(d_pm, d_lens, out, b_begin=b0, b_count=n, position_major=True, chars_pm_stride=stride, stream=s,
                           cells=fr_cells.view(-1)[:ncols * n * M * 4].view(ncols, n, M, 4))

    fr_us = time_graph(fr, rounds, launches)
    fr_written = rows * 32 * ncols
    rate, fr_rate = written / (us * 1e-6), fr_written / (fr_us * 1e-6)
    res = {"call": "inputs", "variant": variant, "shape": label, "B": B, "M": M, "D": D, "window": window, "calls": -(-B // window), "device_us": round(us, 1),
           "bytes_read": read, "bytes_written": written, "fraction_of_8TBps": round((read + written) / (us * 1e-6) / PEAK, 4),
           "cell_bytes_per_s": round(rate / 1e9, 1), "fr_columns_us": round(fr_us, 1), "fr_columns_cell_bytes_per_s": round(fr_rate / 1e9, 1),
           "ratio_to_fr_columns_byte_rate": round(rate / fr_rate, 3), "host_twin_16_threads_ms": round(host_s * 1e3, 1),
           "ratio_to_host_twin": round(host_s * 1e6 / us, 1)}
    print("%-10s %-24s B=%d M=%d D=%d  window %d  device %10.1f us = %.3f of 8 TB/s (%.0f GB/s of cells)   fr_columns %10.1f us (%.0f GB/s of cells): ratio %.3f"
          "   host twin, 16 threads %9.1f ms (%.0f times)" % (variant, label, B, M, D, window, us, res["fraction_of_8TBps"], rate / 1e9, fr_us, fr_rate / 1e9,
                                                              rate / fr_rate, host_s * 1e3, host_s * 1e6 / us), flush=True)
    return res


def run_table(label, variant, names, n_theta, rounds, launches):
    cfg = config(names, 64)
    cfg.set_option(hra.OPT_HOST_THREADS, 16)
    W = cfg.lookup_words()
    theta = random_theta(n_theta, 2)
    d_theta = torch.from_numpy(theta.view(np.int64)).to(DEV)
    cells = torch.empty((n_theta, W, 4), dtype=torch.int64, device=DEV)
    cfg.lookup_compress_table(d_theta, out=cells)
    torch.cuda.synchronize()
    want = np.empty((n_theta, W, 4), np.uint64)
    cfg.lookup_compress_table_host(theta, out=want)
    t0 = time.perf_counter()
    cfg.lookup_compress_table_host(theta, out=want)
    host_s = time.perf_counter() - t0
    if not np.array_equal(cells.cpu().numpy().view(np.uint64), want):
        print("%s: the device table cells differ from the host twin's" % label)
        return None
    us = time_graph(lambda s: cfg.lookup_compress_table(d_theta, out=cells, stream=s), rounds, launches)
    read, written = 16 * W + 32 * n_theta, 32 * W * n_theta
    res = {"call": "table", "variant": variant, "shape": label, "W": W, "n_theta": n_theta, "device_us": round(us, 1), "bytes_read": read, "bytes_written": written,
           "fraction_of_8TBps": round((read + written) / (us * 1e-6) / PEAK, 4), "host_twin_16_threads_ms": round(host_s * 1e3, 2),
           "ratio_to_host_twin": round(host_s * 1e6 / us, 1)}
    print("%-10s table %-18s W=%d n_theta=%d  device %9.1f us = %.3f of 8 TB/s   host twin, 16 threads %8.2f ms (%.0f times)"
          % (variant, label, W, n_theta, us, res["fraction_of_8TBps"], host_s * 1e3, host_s * 1e6 / us), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--label", default="in-place")
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--skip-table", action="store_true")
    args = ap.parse_args()
    shapes = [("regex1", CFG_1, args.B, 1024, synth.regex1_planted, 0), ("regex2 + regex3, windowed", CFG_23, args.B, 2048, synth.regex23_planted, args.B // 4)]
    if not args.skip_long:
        shapes.append(("regex1 long, windowed", CFG_1, args.B // 8, 32768, synth.regex1_planted, args.B // 32))
    results = []
    for label, names, B, M, make, window in shapes:
        r = run_shape(label, args.label, names, B, M, make, window, args.rounds, args.launches)
        if r is None:
            return 1
        results.append(r)
    if not args.skip_table:
        for label, names in (("regex1", CFG_1), ("regex2 + regex3", CFG_23)):
            for n_theta in (1, 4096):
                r = run_table(label, args.label, names, n_theta, args.rounds, args.launches)
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
