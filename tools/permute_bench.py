#!/usr/bin/env python3
"""LOOKUP PERMUTE: hrx_lookup_permute_device on regex1 at 65536 x 1024 and regex2 + regex3 at 65536 x 2048 with n_rows = 4090, pitch 4096, and
regex1 at 8192 x 32768 with n_rows = 65530, pitch 65536 — position-major witness rows, the counts from hrx_lookup_counts_device, in windows of as many
strings as 16 GiB of outputs hold (one call per window; the figure is their sum).  Each shape indices only, and indices plus cells with one table run per
string (hrx_lookup_compress_table_device, one challenge per string of the window).

Method: a graph of `--launches` passes over the windows on one stream, `--rounds` replays, the median, us per pass.  Before anything is timed the device
index columns of the whole shape and the cells of the first --check-cells strings must equal the host twin's (hrx_lookup_permute_host on the counts copied
out, HRX_OPT_HOST_THREADS = 16); the tool stops otherwise.  The host twin's wall time is that of the checked cells' strings, scaled to the shape.

Nobody has measured such a kernel here and no threshold is set.  Per shape and mode: us; the fraction of 8 TB/s over the algorithmic bytes — per lookup 4 T
read, 8 n_rows written, 64 n_rows more with cells; the byte rate of the cells against that of hrx_fr_columns_device on the same rows in the same run; the
ratio to the host twin.  --json FILE: the figures as a JSON list (profiles/permute_bench.json); --label: the name the figures carry, for runs that compare two
libraries through HRX_LIB_PATH."""
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
from halo2_regex_amd import synth  # noqa: E402
from compress_bench import CFG_1, CFG_23, DEV, PEAK, PM_IN, config, random_theta, time_graph  # noqa: E402

OUT_BYTES = 1 << 34           # outputs of one window


def run_shape(label, variant, names, B, M, make, n_rows, pitch, rounds, launches, check_cells):
    cfg = config(names, M)
    cfg.set_option(hra.OPT_HOST_THREADS, 16)
    D, W = cfg.num_defs, cfg.lookup_words()
    ncols = 3 * D
    chars, lens = make(B, M - 8, stride=M + 16)
    stride = chars.shape[1]
    d_pm = hra.chars_to_position_major(torch.from_numpy(chars).to(DEV))
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    out = cfg.witness_batch_position_major(d_pm, d_lens, chars_pm_stride=stride)
    counts, misses = cfg.lookup_counts(d_pm, d_lens, out[0], layout=PM_IN, chars_pm_stride=stride)
    torch.cuda.synchronize()
    window = min(B, max(1, OUT_BYTES // (ncols * pitch * 72)))
    d_theta = torch.from_numpy(random_theta(window, 1).view(np.int64)).to(DEV)
    table = cfg.lookup_compress_table(d_theta)                      # [window][W][4]: run i belongs to string i of every window
    bufs = {"a_idx": torch.empty((ncols, window, pitch), dtype=torch.int32, device=DEV), "s_idx": torch.empty((ncols, window, pitch), dtype=torch.int32, device=DEV),
            "a_cells": torch.empty((ncols, window, pitch, 4), dtype=torch.int64, device=DEV), "s_cells": torch.empty((ncols, window, pitch, 4), dtype=torch.int64, device=DEV),
            "overflow": torch.empty((window,), dtype=torch.int32, device=DEV)}

    def views(n, with_cells):
        v = {k: t.view(-1)[:t.numel() // window * n].view((ncols, n) + tuple(t.shape[2:])) for k, t in bufs.items() if k != "overflow" and (with_cells or "idx" in k)}
        v["overflow"] = bufs["overflow"][:n]
        return v

    def one_window(b0, n, with_cells, s):
        return cfg.lookup_permute(counts[b0:b0 + n], n_rows, table=table[:n] if with_cells else None, pitch=pitch, out=views(n, with_cells), stream=s)

    def device(with_cells):
        def fn(s):
            for b0 in range(0, B, window):
                one_window(b0, min(window, B - b0), with_cells, s)
        return fn

    # the index columns of the whole shape and the cells of the first strings against the host twin
    h_counts = counts.cpu().numpy().view(np.uint32)
    chunk = max(1, min(window, (1 << 29) // (ncols * pitch * 8)))
    for b0 in range(0, B, chunk):
        n = min(chunk, B - b0)
        got = one_window(b0, n, False, torch.cuda.current_stream(DEV))
        torch.cuda.synchronize()
        want = cfg.lookup_permute_host(h_counts[b0:b0 + n], n_rows, pitch=pitch, out=("idx",))
        for k in ("a_idx", "s_idx"):
            if not np.array_equal(got[k].cpu().numpy().view(np.uint32)[:, :, :n_rows], want[k][:, :, :n_rows]):
                print("%s: %s of strings %d .. %d differs from the host twin's" % (label, k, b0, b0 + n))
                return None
        if bool(got["overflow"].any()) or want["overflow"].any():
            print("%s: an overflow bit" % label)
            return None
    n = max(1, min(check_cells, window, (1 << 30) // (ncols * pitch * 64)))
    got = one_window(0, n, True, torch.cuda.current_stream(DEV))
    torch.cuda.synchronize()
    h_table = table[:n].cpu().numpy().view(np.uint64)
    host_s = {}
    for mode, names_out in (("indices", ("idx",)), ("indices + cells", ("idx", "cells"))):
        t0 = time.perf_counter()
        want = cfg.lookup_permute_host(h_counts[:n], n_rows, table=h_table if "cells" in names_out else None, pitch=pitch, out=names_out)
        host_s[mode] = (time.perf_counter() - t0) * B / n
    for k in ("a_cells", "s_cells"):
        if not np.array_equal(got[k].cpu().numpy().view(np.uint64)[:, :, :n_rows], want[k][:, :, :n_rows]):
            print("%s: %s of the first %d strings differs from the host twin's" % (label, k, n))
            return None
    del want, got
    # the yardstick: the field cells of the same rows, in four windows
    fr_cols, fr_window = 4 + 4 * D, max(1, B // 4)
    fr_cells = torch.empty((fr_cols, fr_window, M, 4), dtype=torch.int64, device=DEV)

    def fr(s):
        for b0 in range(0, B, fr_window):
            n = min(fr_window, B - b0)
            cfg.fr_columns(d_pm, d_lens, out, b_begin=b0, b_count=n, position_major=True, chars_pm_stride=stride, stream=s,
                           cells=fr_cells.view(-1)[:fr_cols * n * M * 4].view(fr_cols, n, M, 4))

    fr_us = time_graph(fr, rounds, launches)
    fr_rate = B * M * 32 * fr_cols / (fr_us * 1e-6)
    del fr_cells
    T_sum = sum(sl.stop - sl.start for lay in cfg.lookup_layout() for sl in lay.values())
    plan = cfg.lookup_permute_plan(window, n_rows)
    results = []
    for mode, with_cells in (("indices", False), ("indices + cells", True)):
        us = time_graph(device(with_cells), rounds, launches)
        read, written = B * 4 * T_sum, B * ncols * n_rows * (72 if with_cells else 8)
        res = {"variant": variant, "shape": label, "mode": mode, "B": B, "M": M, "D": D, "n_rows": n_rows, "pitch": pitch, "window": window, "calls": -(-B // window),
               "groups": plan["groups"], "group_rows": plan["group_rows"], "device_us": round(us, 1), "bytes_read": read, "bytes_written": written,
               "fraction_of_8TBps": round((read + written) / (us * 1e-6) / PEAK, 4), "written_bytes_per_s": round(written / (us * 1e-6) / 1e9, 1),
               "fr_columns_us": round(fr_us, 1), "fr_columns_cell_bytes_per_s": round(fr_rate / 1e9, 1),
               "ratio_to_fr_columns_byte_rate": round(written / (us * 1e-6) / fr_rate, 3), "host_twin_16_threads_ms": round(host_s[mode] * 1e3, 1),
               "host_twin_scaled_from_strings": n, "ratio_to_host_twin": round(host_s[mode] * 1e6 / us, 1)}
        print("%-10s %-22s %-16s B=%d n_rows=%d window %d groups %d  device %10.1f us = %.3f of 8 TB/s (%.0f GB/s written)   fr_columns %.0f GB/s of cells: ratio %.3f"
              "   host twin, 16 threads %9.1f ms (%.0f times)" % (variant, label, mode, B, n_rows, window, plan["groups"], us, res["fraction_of_8TBps"],
                                                                  res["written_bytes_per_s"], fr_rate / 1e9, res["ratio_to_fr_columns_byte_rate"],
                                                                  host_s[mode] * 1e3, host_s[mode] * 1e6 / us), flush=True)
        results.append(res)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("--check-cells", type=int, default=1024)
    ap.add_argument("--json", default=None)
    ap.add_argument("--label", default="lookup-group")
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    shapes = [("regex1", CFG_1, args.B, 1024, synth.regex1_planted, 4090, 4096), ("regex2 + regex3", CFG_23, args.B, 2048, synth.regex23_planted, 4090, 4096)]
    if not args.skip_long:
        shapes.append(("regex1 long", CFG_1, args.B // 8, 32768, synth.regex1_planted, 65530, 65536))
    results = []
    for label, names, B, M, make, n_rows, pitch in shapes:
        r = run_shape(label, args.label, names, B, M, make, n_rows, pitch, args.rounds, args.launches, args.check_cells)
        if r is None:
            return 1
        results += r
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
