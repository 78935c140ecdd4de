#!/usr/bin/env python3
"""LOOKUP PRODUCT: hrx_lookup_product_device on regex1 at 65536 x 1024 and regex2 + regex3 at 65536 x 2048 with n_rows = 4090, pitches 4096,
and regex1 at 8192 x 32768 with n_rows = 65530, pitches 65536 — §21's three shapes.  The input cells, the index columns, the tables and the inverse tables
come from the device chain (lookup_counts, lookup_compress_inputs / _table, lookup_permute, lookup_invert_table) on position-major witness rows, one
challenge triple and one table run per string, in windows of as many strings as 8 GiB of buffers hold.  The timed graph runs the product call once per
window of the shape, every call on the buffers of the shape's FIRST window (the arithmetic does not depend on the data; the gathers follow real indices).

Method: a graph of `--launches` passes on one stream, `--rounds` replays, the median, us per pass.  Before anything is timed the device's Z columns and open
words of the first --check strings must equal the host twin's (hrx_lookup_product_host on the buffers copied out, HRX_OPT_HOST_THREADS = 16) and every
honest string must close; the tool stops otherwise.  The host twin's wall time is that of the checked strings, scaled to the shape.

Nobody has measured such a kernel here and no threshold is set.  Per shape: us; the fraction of 8 TB/s over the algorithmic bytes — per row and lookup 32
read (A), 8 read (indices), 32 written; in the same run lookup_permute with cells on the same windows (the nearest launch by bytes written) and
hrx_fr_columns_device on the same rows (the yardstick for cell stores); the ratio to the host twin.  The invert call: one run and 4096 runs of regex1's
table against lookup_compress_table on the same runs, and one run of the synthetic 256-state DFA's 65537-row table; from the two single runs the cost per
tile and what is left at zero tiles — launch and the Fermat step — by a straight line (an inference, said so in the output).  --json FILE: the figures as a
JSON list (profiles/product_bench.json)."""
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

BUF_BYTES = 1 << 33           # buffers of one window


def run_shape(label, variant, names, B, M, make, n_rows, pitch, rounds, launches, check):
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
    per_string = ncols * (M * 32 + pitch * (8 + 32 + 64)) + 3 * W * 32
    window = max(1, min(B, BUF_BYTES // per_string))
    ch = [torch.from_numpy(random_theta(window, seed).view(np.int64)).to(DEV) for seed in (1, 2, 3)]       # theta, beta, gamma of the window's strings
    table = cfg.lookup_compress_table(ch[0])
    inv_beta, inv_gamma = cfg.lookup_invert_table(table, ch[1]), cfg.lookup_invert_table(table, ch[2])
    inputs = cfg.lookup_compress_inputs(d_pm, d_lens, out[0], ch[0], layout=PM_IN, b_begin=0, b_count=window, chars_pm_stride=stride)
    perm = cfg.lookup_permute(counts[:window], n_rows, pitch=pitch, out=("idx",))
    z = torch.empty((ncols, window, pitch, 4), dtype=torch.int64, device=DEV)
    opened = torch.empty((window,), dtype=torch.int32, device=DEV)
    calls = -(-B // window)

    def product(s):
        for _ in range(calls):
            cfg.lookup_product(d_lens, inputs, perm["a_idx"], perm["s_idx"], n_rows, table, inv_beta, inv_gamma, ch[1], ch[2], z_pitch=pitch,
                               out={"z": z, "open": opened}, stream=s)

    product(torch.cuda.current_stream(DEV))
    torch.cuda.synchronize()
    # the first strings against the host twin; every honest string of the window closes
    n = max(1, min(check, window))
    u64, u32 = (lambda t: t.cpu().numpy().view(np.uint64)), (lambda t: t.cpu().numpy().view(np.uint32))
    h = dict(inputs=u64(inputs[:, :n].contiguous()), a=u32(perm["a_idx"][:, :n].contiguous()), s=u32(perm["s_idx"][:, :n].contiguous()), table=u64(table[:n]),
             ib=u64(inv_beta[:n]), ig=u64(inv_gamma[:n]), beta=u64(ch[1][:n]), gamma=u64(ch[2][:n]))
    t0 = time.perf_counter()
    want = cfg.lookup_product_host(lens, h["inputs"], h["a"], h["s"], n_rows, h["table"], h["ib"], h["ig"], h["beta"], h["gamma"], z_pitch=pitch)
    host_s = (time.perf_counter() - t0) * B / n
    if not np.array_equal(u64(z[:, :n].contiguous())[:, :, :n_rows + 1], want["z"][:, :, :n_rows + 1]) or not np.array_equal(u32(opened[:n]), want["open"]):
        print("%s: Z of the first %d strings differs from the host twin's" % (label, n))
        return None
    honest = (u32(misses[:window]) == 0) & (u32(perm["overflow"]) == 0)
    if (u32(opened)[honest] != 0).any() or not honest.any():
        print("%s: an honest string does not close" % label)
        return None
    del want, h
    us = time_graph(product, rounds, launches)
    # lookup_permute with cells on the same windows' counts, into buffers of its own
    cells = {k: torch.empty((ncols, window, pitch, 4), dtype=torch.int64, device=DEV) for k in ("a_cells", "s_cells")}
    cells.update(a_idx=perm["a_idx"], s_idx=perm["s_idx"], overflow=perm["overflow"])

    def permute(s):
        for b0 in range(0, B, window):
            nb = min(window, B - b0)
            v = {k: t.view(-1)[:t.numel() // window * nb].view((ncols, nb) + tuple(t.shape[2:])) if k != "overflow" else t[:nb] for k, t in cells.items()}
            cfg.lookup_permute(counts[b0:b0 + nb], n_rows, table=table[:nb], pitch=pitch, out=v, stream=s)

    perm_us = time_graph(permute, rounds, launches)
    del cells
    fr_cols, fr_window = 4 + 4 * D, max(1, B // 4)
    fr_cells = torch.empty((fr_cols, fr_window, M, 4), dtype=torch.int64, device=DEV)

    def fr(s):
        for b0 in range(0, B, fr_window):
            nb = min(fr_window, B - b0)
            cfg.fr_columns(d_pm, d_lens, out, b_begin=b0, b_count=nb, position_major=True, chars_pm_stride=stride, stream=s,
                           cells=fr_cells.view(-1)[:fr_cols * nb * M * 4].view(fr_cols, nb, M, 4))

    fr_us = time_graph(fr, rounds, launches)
    fr_rate = B * M * 32 * fr_cols / (fr_us * 1e-6)
    rows = calls * window * ncols * n_rows
    read, written = rows * 40, rows * 32
    plan = cfg.lookup_product_plan(window, n_rows)
    res = {"variant": variant, "shape": label, "B": B, "M": M, "D": D, "n_rows": n_rows, "pitch": pitch, "window": window, "calls": calls,
           "tile_rows": plan["tile_rows"], "rows_per_lane": plan["rows_per_lane"], "device_us": round(us, 1), "rows_times_lookups": rows,
           "ns_per_1000_rows": round(us * 1e6 / rows, 2), "bytes_read": read, "bytes_written": written, "fraction_of_8TBps": round((read + written) / (us * 1e-6) / PEAK, 4),
           "written_bytes_per_s": round(written / (us * 1e-6) / 1e9, 1), "permute_with_cells_us": round(perm_us, 1),
           "permute_written_bytes_per_s": round(B * ncols * n_rows * 72 / (perm_us * 1e-6) / 1e9, 1), "fr_columns_us": round(fr_us, 1),
           "fr_columns_cell_bytes_per_s": round(fr_rate / 1e9, 1), "ratio_to_fr_columns_byte_rate": round(written / (us * 1e-6) / fr_rate, 3),
           "host_twin_16_threads_ms": round(host_s * 1e3, 1), "host_twin_scaled_from_strings": n, "ratio_to_host_twin": round(host_s * 1e6 / us, 1)}
    print("%-10s %-18s B=%d n_rows=%d window %d x %d calls  product %10.1f us = %.3f of 8 TB/s (%.0f GB/s written)   permute with cells %10.1f us   fr_columns %.0f GB/s"
          " of cells: ratio %.3f   host twin, 16 threads %9.1f ms (%.0f times)" % (variant, label, B, n_rows, window, calls, us, res["fraction_of_8TBps"],
                                                                                res["written_bytes_per_s"], perm_us, fr_rate / 1e9, res["ratio_to_fr_columns_byte_rate"],
                                                                                host_s * 1e3, host_s * 1e6 / us), flush=True)
    return [res]


def run_invert(variant, rounds, launches):
    """one run and 4096 runs of regex1's table, and one run of the 65537-row table"""
    a_txt, sub_txt = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=200)
    big = hra.RegexVerifyConfig.configure(64, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub_txt)])], device=0)
    results, single = [], {}
    for label, cfg, runs in (("regex1", config(CFG_1, 64), (1, 4096)), ("dfa256", big, (1,))):
        cfg.set_option(hra.OPT_HOST_THREADS, 16)
        W = cfg.lookup_words()
        tile = cfg.lookup_product_plan(1, 1 << 20)["tile_rows"]
        for n_runs in runs:
            theta = random_theta(n_runs, 2)
            d_theta, d_shift = (torch.from_numpy(random_theta(n_runs, seed).view(np.int64)).to(DEV) for seed in (2, 3))
            table = cfg.lookup_compress_table(d_theta)
            inv = torch.empty_like(table)
            cfg.lookup_invert_table(table, d_shift, out=inv)
            torch.cuda.synchronize()
            n = min(n_runs, 64)
            t0 = time.perf_counter()
            want = cfg.lookup_invert_table_host(table[:n].cpu().numpy().view(np.uint64), d_shift[:n].cpu().numpy().view(np.uint64))
            host_s = (time.perf_counter() - t0) * n_runs / n
            if not np.array_equal(inv[:n].cpu().numpy().view(np.uint64), want):
                print("invert %s: differs from the host twin's" % label)
                return None
            us = time_graph(lambda s: cfg.lookup_invert_table(table, d_shift, out=inv, stream=s), rounds, launches)
            table_us = time_graph(lambda s: cfg.lookup_compress_table(d_theta, out=table, stream=s), rounds, launches)
            tiles = -(-W // tile)
            if n_runs == 1:
                single[label] = (us, tiles)
            res = {"variant": variant, "shape": "invert " + label, "n_runs": n_runs, "W": W, "tiles_per_run": tiles, "device_us": round(us, 1),
                   "compress_table_us": round(table_us, 1), "host_twin_16_threads_ms": round(host_s * 1e3, 2)}
            print("%-10s invert %-8s runs %5d W %6d (%2d tiles)  %9.1f us   lookup_compress_table %9.1f us   host twin, 16 threads %8.2f ms"
                  % (variant, label, n_runs, W, tiles, us, table_us, host_s * 1e3), flush=True)
            results.append(res)
    (u1, t1), (u2, t2) = single["regex1"], single["dfa256"]
    per_tile = (u2 - u1) / (t2 - t1)
    rest = u1 - per_tile * t1
    print("%-10s invert: %.1f us per tile of one run (both passes); %.1f us left at zero tiles — one launch and the Fermat step (a straight line through two runs: an inference)"
          % (variant, per_tile, rest), flush=True)
    results.append({"variant": variant, "shape": "invert, inferred", "us_per_tile": round(per_tile, 2), "us_at_zero_tiles_launch_and_fermat": round(rest, 1)})
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("--check", type=int, default=256)
    ap.add_argument("--json", default=None)
    ap.add_argument("--label", default="rows-per-lane-4")
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--skip-invert", action="store_true")
    args = ap.parse_args()
    shapes = [("regex1", CFG_1, args.B, 1024, synth.regex1_planted, 4090, 4096), ("regex2 + regex3", CFG_23, args.B, 2048, synth.regex23_planted, 4090, 4096)]
    if not args.skip_long:
        shapes.append(("regex1 long", CFG_1, args.B // 8, 32768, synth.regex1_planted, 65530, 65536))
    results = []
    if not args.skip_invert:
        r = run_invert(args.label, args.rounds, args.launches)
        if r is None:
            return 1
        results += r
    for label, names, B, M, make, n_rows, pitch in shapes:
        r = run_shape(label, args.label, names, B, M, make, n_rows, pitch, args.rounds, args.launches, args.check)
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
