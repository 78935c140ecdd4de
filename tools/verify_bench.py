#!/usr/bin/env python3
"""VERIFY against the witness launch that wrote the same rows: hrx_verify_rows_device* on the headline shape — regex1, 65536 x 1024 — and on the
three header defs at 65536 x 2048, position-major interleaved records and record planes, position-major input; --long adds regex1 at 8192 x 32768 (few long
strings: one lane per string leaves most of the device idle — measured, not built for).

Method: every kind is a graph of 10 launches on one stream; the kinds take turns in one process, 20 rounds, medians, us per launch.  The yardstick is the
witness launch on the same buffers (it moves the same bytes the other way), timed twice — the two figures' difference is the noise floor — and the ratio is
against the smaller; hrx_traffic_pass_device* over the same buffers is the no-compute floor.  The order inside a round is witness, verify, witness, traffic
pass: the traffic pass overwrites the rows, the witness launch behind it puts them back before the next verify.  Before anything is timed, every verdict of a
string the witness call accepted (status code 0, every def's accept bit, or n = M) must be 0; the tool stops otherwise.  --torch: the torch checker
(tests/mock_prover.py) on the headline rows, time and peak device memory — what a caller had before.

MI355X, 2026-10-19, one lease, us per launch, witness (its two figures) / traffic pass / verify = verify over the smaller witness figure:
  regex1 65536 x 1024        interleaved  66.6 67.1 /  68.2 /  555.6 = 8.35    row stripes  67.2 67.9 /  67.8 /  563.4 = 8.39
  header defs 65536 x 2048   interleaved 311.6 314.6 / 300.8 / 2611.9 = 8.38   planes      281.7 285.3 / 286.5 / 2659.7 = 9.44
  regex1 8192 x 32768        interleaved 433.5 439.1 / 1226.6 / 15789.7 = 36.4
  torch checker, regex1 65536 x 1024: 26.4 ms, 16.75 GiB of temporaries
The launch is bound by one wave per SIMD issuing 160 instructions a row, not by memory (DESIGN.md §17 has the counters).

--chunked: the chunked verify (hrx_verify_rows_chunked_device*) beside the unchunked launch, same procedure, every chunked verdict equal to the
unchunked launch's before anything is timed, the unchunked launch and the witness launch each timed twice: regex1 at 8192 x 32768 interleaved and the three
header defs at 32768 x 32768 in planes at the context's pick (--long-headers-B: another string count, 0 leaves the shape out), the two headline rows at
K = 1, 2, 4 and the pick.  --floor-sweep: regex1 x 32768 rows, 8192 and 1024 strings, chunks of 128 .. 4096 rows (the floor of hrx_ctx_verify_chunk_rows).
MI355X, 2026-10-20, us per call (two launches), chunked / unchunked / their ratio:
  regex1 8192 x 32768, the pick 2048 (K = 16)        1823.4 / 15765.7 = 0.116 (8.65 times as fast; 4.11 of the witness launch)
  header defs 32768 x 32768, the pick 8192 (K = 4)  15642.8 / 41112.6 = 0.380
  regex1 65536 x 1024        K = 1 821.6   K = 2 482.7 (the pick)   K = 4 482.3   unchunked 542.9
  header defs 65536 x 2048   K = 1 3228.1  K = 2 1958.2 (the pick)  K = 4 1939.1  unchunked 2597.5"""
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
CFG_H3 = [HDR("header_from", 1), HDR("header_to", 1), HDR("header_subject", 3)]
DEV = torch.device("cuda", 0)
PM_IN = hra.LAYOUT_POSITION_MAJOR | hra.LAYOUT_INPUT_POSITION_MAJOR


def config(names, M):
    defs = [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(os.path.join(DFA, a)), [hra.SubstrRegexDef.read_from_text(os.path.join(DFA, s)) for s in subs])
            for a, subs in names]
    return hra.RegexVerifyConfig.configure(M, defs, device=0)


def time_kinds(kinds, rounds=20, launches=10):
    """kinds: name -> fn(stream), in the order they take their turns; -> name -> median microseconds per launch"""
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


def run_shape(label, names, B, M, make, planes, rounds, chunks=()):
    """chunks: chunk_rows values of the chunked verify to time beside the unchunked launch (0: the context's pick); with any, the unchunked launch is timed twice"""
    cfg = config(names, M)
    D = cfg.num_defs
    chars, lens = make(B, M - 8, stride=M + 16)
    stride = chars.shape[1]
    d_pm = hra.chars_to_position_major(torch.from_numpy(chars).to(DEV))
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    if planes:
        out = cfg.alloc_output_planes(B, DEV, stripes=2 if D == 1 else None)
        witness = lambda s: cfg.witness_batch_planes(d_pm, d_lens, out=out, stream=s, chars_pm_stride=stride)
        traffic = lambda s: cfg.traffic_pass_planes(d_pm, B, out, stride, stream=s)
        vkw = dict(planes=out[0])
    else:
        out = cfg.alloc_outputs_position_major(B, DEV)
        witness = lambda s: cfg.witness_batch_position_major(d_pm, d_lens, out=out, stream=s, chars_pm_stride=stride)
        traffic = lambda s: cfg.traffic_pass(d_pm, B, out, stride, stream=s)
        vkw = {}
    verdict = torch.empty((B,), dtype=torch.int64, device=DEV)
    verify = lambda s: cfg.verify_rows(d_pm, d_lens, None if planes else out[0], out[1], layout=PM_IN, out=verdict, chars_pm_stride=stride, stream=s, **vkw)
    chunked = {}
    for c in chunks:
        rows_c = c if c else cfg.verify_chunk_rows(B)
        ws = torch.empty((max(16, hra.verify_chunked_workspace_bytes(B, M, rows_c)),), dtype=torch.uint8, device=DEV)
        v_c = torch.empty((B,), dtype=torch.int64, device=DEV)
        name = "chunked %d%s" % (rows_c, " (the pick)" if not c else "")
        fn = lambda s, c=c, ws=ws, v_c=v_c: cfg.verify_rows(d_pm, d_lens, None if planes else out[0], out[1], layout=PM_IN, out=v_c, chars_pm_stride=stride, stream=s,
                                                            chunk_rows=c, workspace=ws, **vkw)
        chunked[name] = (fn, v_c, -(-M // rows_c))
    s0 = torch.cuda.current_stream(DEV)
    witness(s0)
    verify(s0)
    for fn, v_c, _ in chunked.values():
        fn(s0)
    torch.cuda.synchronize()
    for name, (fn, v_c, _) in chunked.items():
        if not torch.equal(v_c, verdict):
            b = int(torch.nonzero(v_c != verdict)[0])
            print("%s: %s: string %d: %s, the unchunked launch says %s" % (label, name, b, hra.explain_verdict(int(v_c[b])), hra.explain_verdict(int(verdict[b]))))
            return 1
    st = out[2].cpu().numpy().view(np.uint64)
    accepted = ((st & np.uint64(0xff)) == 0) & ((((st >> np.uint64(8)) & np.uint64(0xff)) == np.uint64((1 << D) - 1)) | (lens >= M))
    v = verdict.cpu().numpy().view(np.uint64)
    if (v[accepted] != 0).any():
        b = int(np.nonzero(accepted & (v != 0))[0][0])
        print("%s: string %d was accepted and its rows fail: %s" % (label, b, hra.explain_verdict(v[b])))
        return 1
    kinds = {"witness": witness, "verify": verify}
    kinds.update({name: fn for name, (fn, _, _) in chunked.items()})
    kinds["witness again"] = witness
    if chunked:
        kinds["verify again"] = verify
    kinds["traffic pass"] = traffic
    t = time_kinds(kinds, rounds=rounds)
    witness(s0)
    verify(s0)
    torch.cuda.synchronize()
    if not np.array_equal(verdict.cpu().numpy().view(np.uint64), v):
        print("%s: the verdicts changed between two runs" % label)
        return 1
    w = min(t["witness"], t["witness again"])
    gb = B * M * (1 + 4 * D + 2) / 1e9
    print("%-34s B=%d M=%d D=%d  accepted %d of %d, nonzero verdicts %d  witness %8.1f / %8.1f us  verify %8.1f us = %.3f of it (%.0f GB/s of rows read)  "
          "traffic pass %8.1f us" % (label, B, M, D, int(accepted.sum()), B, int((v != 0).sum()), t["witness"], t["witness again"], t["verify"], t["verify"] / w,
                                     gb / (t["verify"] * 1e-6), t["traffic pass"]), flush=True)
    if chunked:
        u = min(t["verify"], t["verify again"])
        print("    unchunked verify %8.1f / %8.1f us" % (t["verify"], t["verify again"]))
        for name, (_, _, K) in chunked.items():
            print("    %-26s K=%-4d %8.1f us = %.3f of the unchunked launch (%.2f times as fast), %.2f of the witness launch" % (
                name, K, t[name], t[name] / u, u / t[name], t[name] / w), flush=True)
    return 0


def torch_checker(B, M):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mock_prover import IntegerMockProver
    cfg = config(CFG_1, M)
    chars, lens = synth.regex1_planted(B, M - 8, stride=M + 16)
    d_chars, d_lens = torch.from_numpy(chars).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV)
    out = cfg.witness_batch_position_major(d_chars, d_lens)
    rec, msk = hra.position_major_to_string_major(out[0], out[1], B, M, 1)
    mp = IntegerMockProver.from_config(cfg, DEV)
    for _ in range(2):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        code = mp.verify(d_chars, d_lens, rec, msk, M)
        b.record()
        b.synchronize()
        ms, peak = a.elapsed_time(b), torch.cuda.max_memory_allocated(DEV) - base
    v = cfg.verify_rows(d_chars, d_lens, out[0], out[1], layout=hra.LAYOUT_POSITION_MAJOR)
    same = torch.equal(v & 0xffffffff, code)
    print("torch checker, regex1 B=%d M=%d: %.1f ms, peak %.2f GiB above the rows; its bits %s verify_rows'" % (B, M, ms, peak / 2 ** 30, "equal" if same else "DIFFER FROM"), flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--long", action="store_true", help="also regex1 at 8192 x 32768")
    ap.add_argument("--torch", action="store_true", help="also the torch checker on the headline rows")
    ap.add_argument("--chunked", action="store_true", help="the chunked verify instead: few long strings at the context's pick, the headline rows at K = 1, 2, 4 and the pick")
    ap.add_argument("--floor-sweep", action="store_true", help="the chunked verify at chunks of 128 .. 4096 rows, regex1 x 32768 rows, 8192 and 1024 strings")
    ap.add_argument("--long-headers-B", type=int, default=32768, help="--chunked: strings of the three header defs x 32768 rows (0: leave the shape out)")
    args = ap.parse_args()
    rc = 0
    long_rounds = max(4, args.rounds // 4)
    if args.floor_sweep:
        sweep = (128, 256, 512, 1024, 2048, 4096, 0)
        rc |= run_shape("regex1 long, interleaved", CFG_1, args.B // 8, 32768, synth.regex1_planted, False, long_rounds, chunks=sweep)
        rc |= run_shape("regex1 long, 1024 strings", CFG_1, args.B // 64, 32768, synth.regex1_planted, False, long_rounds, chunks=sweep)
        return rc
    if args.chunked:
        rc |= run_shape("regex1 long, interleaved", CFG_1, args.B // 8, 32768, synth.regex1_planted, False, long_rounds, chunks=(0,))
        rc |= run_shape("regex1 interleaved", CFG_1, args.B, 1024, synth.regex1_planted, False, args.rounds, chunks=(1024, 512, 256, 0))
        rc |= run_shape("three header defs interleaved", CFG_H3, args.B, 2048, synth.headers_planted, False, args.rounds, chunks=(2048, 1024, 512, 0))
        if args.long_headers_B:
            rc |= run_shape("three header defs long, planes", CFG_H3, args.long_headers_B, 32768, synth.headers_planted, True, long_rounds, chunks=(0,))
        return rc
    for planes in (False, True):
        rc |= run_shape("regex1 " + ("row stripes" if planes else "interleaved"), CFG_1, args.B, 1024, synth.regex1_planted, planes, args.rounds)
        rc |= run_shape("three header defs " + ("planes" if planes else "interleaved"), CFG_H3, args.B, 2048, synth.headers_planted, planes, args.rounds)
    if args.long:
        rc |= run_shape("regex1 long, interleaved", CFG_1, args.B // 8, 32768, synth.regex1_planted, False, max(4, args.rounds // 4))
    if args.torch:
        rc |= torch_checker(args.B, 1024)
    return rc


if __name__ == "__main__":
    sys.exit(main())
