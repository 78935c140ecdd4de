#!/usr/bin/env python3
"""LOOKUP QUOTIENT: hrx_lookup_quotient_device over §23's three window shapes — regex1 at 65536 x 1024 (k = 12, 3 lookups a string), regex2 +
regex3 at 65536 x 2048 (k = 12, 6 lookups a string) and regex1 at 8192 x 32768 (k = 16, 3 lookups a string) — at ext_k = k + 2, canonical limbs, h_in absent,
the division on, one table run for the call.  The columns are seeded field elements: the arithmetic does not depend on the data.  A call takes as many
strings as --buf-bytes of input columns hold (A, A', S', Z: 4 x lookups x 2^ext_k cells a string); every timed call runs on the buffers of the first window.

Method: a graph of one pass over the shape's strings on one stream, `--rounds` replays, the median.  Before anything is timed the first --check strings
(at most a call's window) must equal the host twin's (hrx_lookup_quotient_host, HRX_OPT_HOST_THREADS = 16); the tool stops otherwise.  The host twin's wall
time is that of the checked strings, scaled to the shape.

Nothing earlier computes this on the device and no threshold is set.  What matters is the cost beside what already feeds the stage: in the same run, the
extended forward transform (hrx_fr_ntt_device at ext_k, n_in = 2^k, a shift) of the five input columns of every lookup — one window's worth timed the
same way and scaled to the shape's strings.  Recorded: the
quotient's us per pass and its ratio to that transform time, ps per point and lookup, the fraction of 8 TB/s over the algorithmic bytes (every input cell
read once, every h cell written once), the fr_mul rate the rule's product count implies (12 a point and lookup, 4 + 1 a point) — arithmetic, an INFERENCE,
not a counter; so is every byte figure — and the host twin on 16 threads.  --json FILE: the figures as a JSON list (profiles/quotient_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import halo2_regex_amd as hra  # noqa: E402
from compress_bench import CFG_1, CFG_23, DEV, PEAK, config, time_graph  # noqa: E402
from ntt_bench import random_cells  # noqa: E402

FR_MUL_PER_POINT_AND_LOOKUP, FR_MUL_PER_POINT = 12, 5      # csrc/hrx_quotient.hpp: the fold; the four brackets and the division


def run_shape(cfg, label, variant, strings, k, buf_bytes, rounds, check):
    ncols, ext_k = 3 * cfg.num_defs, k + 2
    n, N = 1 << k, 1 << ext_k
    window = max(1, min(strings, buf_bytes // (4 * ncols * N * 32)))
    calls = -(-strings // window)
    seven = torch.tensor([7, 0, 0, 0], dtype=torch.int64, device=DEV)        # the plain 7: the calls are canonical
    cols = [random_cells(ncols * window, N, 10 + i).view(ncols, window, N, 4) for i in range(4)]      # A, A', S', Z
    s_ext, sel = random_cells(ncols, N, 20), random_cells(3, N, 21)
    ch = random_cells(1, 3, 22)[0]
    t_inv = cfg.fr_vanishing_inverse(k, ext_k, seven, canonical=True)
    h = torch.empty((window, N, 4), dtype=torch.int64, device=DEV)

    def run(s):
        for _ in range(calls):
            cfg.lookup_quotient(k, ext_k, cols[0], cols[1], cols[2], cols[3], s_ext, sel, ch[0], ch[1], ch[2], out=h, t_inv=t_inv, divide=True, canonical=True, stream=s)

    run(torch.cuda.current_stream(DEV))
    torch.cuda.synchronize()
    c = min(check, window)
    host = lambda t: t.cpu().numpy().view(np.uint64)
    args = [np.ascontiguousarray(host(t[:, :c])) for t in cols] + [host(s_ext), host(sel), host(ch[0]), host(ch[1]), host(ch[2])]
    t0 = time.perf_counter()
    want = cfg.lookup_quotient_host(k, ext_k, *args, t_inv=host(t_inv), divide=True, canonical=True)
    host_s = (time.perf_counter() - t0) * strings / c
    if not np.array_equal(host(h[:c]), want):
        print("%s: the first %d strings differ from the host twin's" % (label, c))
        return None
    del want, args
    us = time_graph(run, rounds, 1)
    # what feeds the stage: the extended forward transform of five columns a lookup (the table's once a call)
    ws = cfg.fr_ntt_prepare(ext_k)
    src = random_cells(ncols * window, n, 30)
    dst = cols[0].view(ncols * window, N, 4)

    def ntt(s):                              # one window's worth: the calls of a pass are alike, and §23 has the whole pass
        for _ in range(4):
            cfg.fr_ntt(src, ext_k, workspace=ws, out=dst, n_in=n, shift=seven, canonical=True, stream=s)
        cfg.fr_ntt(src[:ncols], ext_k, workspace=ws, out=dst[:ncols], n_in=n, shift=seven, canonical=True, stream=s)

    ntt_us = time_graph(ntt, rounds, 1) * strings / window
    points = strings * N
    algorithmic = (4 * ncols * strings * N + calls * (ncols + 3) * N + strings * N) * 32
    fr_mul = points * (FR_MUL_PER_POINT_AND_LOOKUP * ncols + FR_MUL_PER_POINT)
    res = {"variant": variant, "shape": label, "k": k, "ext_k": ext_k, "lookups": ncols, "strings": strings, "strings_per_call": window, "calls": calls,
           "device_us": round(us, 1), "us_per_call": round(us / calls, 1), "ps_per_point_and_lookup": round(us * 1e6 / (points * ncols), 2),
           "extended_ntt_of_the_inputs_us": round(ntt_us, 1), "extended_ntt_scaled_from_strings": window, "ratio_to_extended_ntt": round(us / ntt_us, 3), "algorithmic_bytes": algorithmic,
           "fraction_of_8TBps": round(algorithmic / (us * 1e-6) / PEAK, 4), "fr_mul_per_point_and_lookup": FR_MUL_PER_POINT_AND_LOOKUP,
           "fr_mul_per_s_inferred": round(fr_mul / (us * 1e-6) / 1e9, 1), "host_twin_16_threads_ms": round(host_s * 1e3, 1), "host_twin_scaled_from_strings": c,
           "ratio_to_host_twin": round(host_s * 1e6 / us, 1)}
    print("%-10s %-16s k=%2d lookups %d strings %6d in %3d calls  %10.1f us  %6.2f ps/point/lookup  %.3f of the extended NTT of its inputs (%.1f us)  %.3f of 8 TB/s"
          "  %.1f G fr_mul/s (inferred)  host twin, 16 threads %9.1f ms (%.0f times)"
          % (variant, label, k, ncols, strings, calls, us, res["ps_per_point_and_lookup"], res["ratio_to_extended_ntt"], ntt_us, res["fraction_of_8TBps"],
             res["fr_mul_per_s_inferred"], host_s * 1e3, host_s * 1e6 / us), flush=True)
    return [res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--check", type=int, default=256)
    ap.add_argument("--buf-bytes", type=int, default=1 << 32)
    ap.add_argument("--json", default=None)
    ap.add_argument("--label", default="tile-256-lds-halo")
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    shapes = [("regex1", CFG_1, args.B, 12), ("regex2 + regex3", CFG_23, args.B, 12)]
    if not args.skip_long:
        shapes.append(("regex1 long", CFG_1, args.B // 8, 16))
    results = []
    for label, names, strings, k in shapes:
        cfg = config(names, 64)              # the stage reads nothing of the defs but their number
        cfg.set_option(hra.OPT_HOST_THREADS, 16)
        r = run_shape(cfg, label, args.label, strings, k, args.buf_bytes, args.rounds, args.check)
        if r is None:
            return 1
        results += r
        del cfg
        torch.cuda.empty_cache()
        if args.json:
            with open(args.json, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
