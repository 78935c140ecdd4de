#!/usr/bin/env python3
"""FR NTT: hrx_fr_ntt_device over the columns of §21's three window shapes — regex1 at 65536 x 1024 (k = 12, 3 columns a string), regex2 +
regex3 at 65536 x 2048 (k = 12, 6 columns a string) and regex1 at 8192 x 32768 (k = 16, 3 columns a string), three kinds of column each (A', S', Z).  Per
shape: the inverse transform in place (lagrange_to_coeff) over all columns, in calls of as many columns as --buf-bytes hold, and the extended forward
transform at k + 2 with n_in = 2^k and shift 7 (coeff_to_extended) into a buffer of its own.  The cells are seeded field elements: the arithmetic does not
depend on the data.  Every timed call runs on the buffers of the shape's first window.

Method: a graph of `--launches` passes on one stream, `--rounds` replays, the median, us per pass.  Before anything is timed the first --check columns of both
transforms must equal the host twin's (hrx_fr_ntt_host, HRX_OPT_HOST_THREADS = 16); the tool stops otherwise.  The host twin's wall time is that of the
checked columns, scaled to the shape.

Nothing earlier exists to compare with and no threshold is set.  Recorded per transform: us per pass, ps per output cell, the fraction of 8 TB/s over the
algorithmic bytes (every input cell read once, every output cell written once — what the call cannot avoid; a multi-pass call moves more: launches x 64
bytes a cell, recorded beside it), the ratio of that byte rate to hrx_fr_columns_device's cell stores measured in the same run (regex1 rows, position-major),
the ratio to the host twin, and the fr_mul count per output cell the rule implies — arithmetic over the plan, an INFERENCE, not a counter; so is every byte
figure.  --json FILE: the figures as a JSON list (profiles/ntt_bench.json)."""
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
from compress_bench import CFG_1, DEV, PEAK, config, time_graph  # noqa: E402


def random_cells(n_cols, n, seed):
    """int64 CUDA limbs [n_cols][n][4] of elements below 2^252 (fully reduced in either limb form)"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    t = torch.randint(0, 1 << 62, (n_cols, n, 4), dtype=torch.int64, device=DEV, generator=g)
    t[:, :, 3] >>= 2
    return t


def fr_mul_per_cell(k, shifted, inverse):
    """what the rule implies per OUTPUT cell: half a product per stage; one for the inverse's scaling, or for the shift (the forward shift runs over every
    cell of the first pass's tiles, zero or not); with a shift the first powers by square-and-multiply, one per lane and tile (eight cells, fewer in the
    smaller tiles), about 1.5 products per bit of the index"""
    return round(k / 2.0 + (1.0 if inverse or shifted else 0.0) + (1.5 * k / 8.0 if shifted else 0.0), 2)


def fr_columns_rate(rounds, launches, B=16384, M=1024):
    cfg = config(CFG_1, M)
    chars, lens = synth.regex1_planted(B, M - 8, stride=M + 16)
    stride = chars.shape[1]
    d_pm = hra.chars_to_position_major(torch.from_numpy(chars).to(DEV))
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    out = cfg.witness_batch_position_major(d_pm, d_lens, chars_pm_stride=stride)
    cols = 4 + 4 * cfg.num_defs
    cells = torch.empty((cols, B, M, 4), dtype=torch.int64, device=DEV)
    us = time_graph(lambda s: cfg.fr_columns(d_pm, d_lens, out, position_major=True, chars_pm_stride=stride, stream=s, cells=cells), rounds, launches)
    return B * M * 32 * cols / (us * 1e-6)


def run_shape(cfg, label, variant, n_cols_total, k, buf_bytes, rounds, launches, check, fr_rate):
    results = []
    seven = torch.tensor([7, 0, 0, 0], dtype=torch.int64, device=DEV)        # the plain 7: the calls are canonical (no cost per cell, hrx_ntt.hpp)
    for what, kk, n_in, inverse, shift in (("inverse, in place", k, 1 << k, True, None), ("extended forward, shift 7", k + 2, 1 << k, False, seven)):
        n, plan = 1 << kk, cfg.fr_ntt_plan(1, kk)
        window = max(1, min(n_cols_total, buf_bytes // (n * 32)))
        calls = -(-n_cols_total // window)
        ws = cfg.fr_ntt_prepare(kk)
        src = random_cells(window, n_in, kk)
        dst = src if inverse else torch.empty((window, n, 4), dtype=torch.int64, device=DEV)
        c = min(check, window)
        keep = src[:c].clone()
        chk = keep.clone()                   # one call on the first columns, for the comparison (the timed calls transform their buffer over and over)
        chk = cfg.fr_ntt(chk, kk, workspace=ws, out=chk if inverse else None, inverse=inverse, n_in=n_in, shift=shift, canonical=True)

        def run(s):
            for _ in range(calls):
                cfg.fr_ntt(src, kk, workspace=ws, out=dst, inverse=inverse, n_in=n_in, shift=shift, canonical=True, stream=s)

        run(torch.cuda.current_stream(DEV))
        torch.cuda.synchronize()
        host_in = keep.cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        want = cfg.fr_ntt_host(host_in, kk, inverse=inverse, n_in=n_in, shift=None if shift is None else shift.cpu().numpy().view(np.uint64), canonical=True)
        host_s = (time.perf_counter() - t0) * n_cols_total / c
        if not np.array_equal(chk.cpu().numpy().view(np.uint64), want):
            print("%s, %s: the first %d columns differ from the host twin's" % (label, what, c))
            return None
        del want
        us = time_graph(run, rounds, launches)
        cells_out = n_cols_total * n
        algorithmic = n_cols_total * (n_in + n) * 32
        launches_per_call = 1 if plan["n_passes"] == 1 else 1 + plan["n_passes"]
        moved = algorithmic if plan["n_passes"] == 1 else n_cols_total * ((n_in + n) + 2 * n * plan["n_passes"]) * 32
        rate = algorithmic / (us * 1e-6)
        res = {"variant": variant, "shape": label, "transform": what, "k": kk, "n_in": n_in, "columns": n_cols_total, "columns_per_call": window, "calls": calls,
               "n_passes": plan["n_passes"], "pass_bits": plan["pass_bits"], "launches_per_call": launches_per_call, "device_us": round(us, 1),
               "us_per_call": round(us / calls, 1), "ps_per_output_cell": round(us * 1e6 / cells_out, 2), "algorithmic_bytes": algorithmic,
               "fraction_of_8TBps": round(rate / PEAK, 4), "bytes_moved_by_all_launches_inferred": moved,
               "fraction_of_8TBps_over_moved_bytes_inferred": round(moved / (us * 1e-6) / PEAK, 4), "fr_columns_cell_bytes_per_s": round(fr_rate / 1e9, 1),
               "ratio_to_fr_columns_byte_rate": round(rate / fr_rate, 3), "host_twin_16_threads_ms": round(host_s * 1e3, 1), "host_twin_scaled_from_columns": c,
               "ratio_to_host_twin": round(host_s * 1e6 / us, 1), "fr_mul_per_output_cell_inferred": fr_mul_per_cell(kk, shift is not None, inverse),
               "fr_mul_per_s_inferred": round(fr_mul_per_cell(kk, shift is not None, inverse) * cells_out / (us * 1e-6) / 1e9, 1)}
        print("%-10s %-16s %-26s k=%2d columns %7d in %3d calls, %d launches each  %10.1f us  %7.2f ps/cell  %.3f of 8 TB/s (%.3f over moved bytes)  %.3f of fr_columns'"
              " rate  host twin, 16 threads %9.1f ms (%.0f times)  %.1f fr_mul/cell -> %.0f G fr_mul/s (inferred)"
              % (variant, label, what, kk, n_cols_total, calls, launches_per_call, us, res["ps_per_output_cell"], res["fraction_of_8TBps"],
                 res["fraction_of_8TBps_over_moved_bytes_inferred"], res["ratio_to_fr_columns_byte_rate"], host_s * 1e3, host_s * 1e6 / us,
                 res["fr_mul_per_output_cell_inferred"], res["fr_mul_per_s_inferred"]), flush=True)
        results.append(res)
        del src, dst, keep, chk
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("--check", type=int, default=256)
    ap.add_argument("--buf-bytes", type=int, default=1 << 32)
    ap.add_argument("--json", default=None)
    ap.add_argument("--label", default="radix-2-lds-4096")
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    cfg = config(CFG_1, 64)                  # the transform reads nothing of the defs
    cfg.set_option(hra.OPT_HOST_THREADS, 16)
    fr_rate = fr_columns_rate(args.rounds, args.launches)
    print("fr_columns' cell stores, regex1 16384 x 1024 position-major: %.0f GB/s" % (fr_rate / 1e9), flush=True)
    shapes = [("regex1", 3 * args.B, 12), ("regex2 + regex3", 6 * args.B, 12)]
    if not args.skip_long:
        shapes.append(("regex1 long", 3 * (args.B // 8), 16))
    results = []
    for label, n_cols, k in shapes:
        r = run_shape(cfg, label, args.label, n_cols, k, args.buf_bytes, args.rounds, args.launches, args.check, fr_rate)
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
