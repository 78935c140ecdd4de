"""SELECTED (include/hrx.h hrx_match_selected_device) measured the way tools/route_bench.py measures: HIP events around a captured graph of K launches of one
kind, the kinds taking turns in one process, medians over --steps intervals; every result is compared with the unselected call's after the timed region.
One JSON line per part and mix:

  unchanged  match_batch_ragged of this build against the same entry point of another build of the library (--parent-lib PATH, loaded beside this one and
             timed twice: the spread between its two runs is the yardstick)
  index      match_selected with sel = arange(B) against the unindexed ragged match on the same input, ragged and string-major source
  ordered    route(status=None, 8 equal length cuts) + match_selected over its order in one graph, against the plain ragged match and the padded match;
             --big also once at 4 B strings with the order ascending and descending
  cascade    the four-def set (via rows) on every string against the same on the survivors of a regex1 screen (route require_accept=1), and the whole
             cascade screen + route + selected second screen

  python tools/select_bench.py [--parts unchanged,index,ordered,cascade] [--parent-lib PATH] [--mixes all_M,uniform,skewed] [--B 65536] [--M 1024] [--big]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import halo2_regex_amd as hra  # noqa: E402
from oracle_lib import DFA_DIR  # noqa: E402
from ragged_bench import timed  # noqa: E402
from route_bench import R1, OtherLib, alloc_match, alloc_route, corpus  # noqa: E402

HDR = lambda n, ns: [n + "_lookup.txt", ["%s_substr%d.txt" % (n, k) for k in range(ns)]]
H4 = [HDR("header_from", 1), HDR("header_to", 1), HDR("header_subject", 3), R1]


def configure(names, M):
    defs = [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(os.path.join(DFA_DIR, a)), [hra.SubstrRegexDef.read_from_text(os.path.join(DFA_DIR, s)) for s in subs])
            for a, subs in names]
    return hra.RegexVerifyConfig.configure(M, defs, device=0)


def same(a, b, idx=None):
    """status, counts and the runs the counts cover, of every string (or of the strings idx)"""
    torch.cuda.synchronize()
    a, b = [t.cpu().numpy() for t in a], [t.cpu().numpy() for t in b]
    if idx is not None:
        a, b = [t[idx] for t in a], [t[idx] for t in b]
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                and hra.decode_spans(a[1].view(np.uint32), a[2].view(np.uint64)) == hra.decode_spans(b[1].view(np.uint32), b[2].view(np.uint64)))


class ParentMatch(OtherLib):
    """hrx_match_batch_device_ragged of another build (route_bench.OtherLib loads it and makes its context)"""

    def __init__(self, path, names, device):
        super().__init__(path, names, device)
        f = self.lib.hrx_match_batch_device_ragged
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]

    def match_batch_ragged(self, values, offsets, M, max_spans, out):
        rc = self.lib.hrx_match_batch_device_ragged(self.ctx, values.data_ptr(), offsets.data_ptr(), offsets.numel() - 1, M, out[0].data_ptr(), out[1].data_ptr(),
                                                    out[2].data_ptr(), max_spans, torch.cuda.current_stream(values.device).cuda_stream)
        assert rc == 0, rc


def part_unchanged(mix, args, cfg, dev):
    B, M, K = args.B, args.M, args.max_spans
    _, _, d_vals, d_offs = corpus(mix, B, M, dev)
    outs = {k: alloc_match(B, K, dev) for k in ("new", "parent_a", "parent_b")}
    other = ParentMatch(args.parent_lib, [R1], 0)
    kinds = {"parent_a": lambda i: other.match_batch_ragged(d_vals, d_offs, M, K, outs["parent_a"]),
             "new": lambda i: cfg.match_batch_ragged(d_vals, d_offs, max_spans=K, out=outs["new"]),
             "parent_b": lambda i: other.match_batch_ragged(d_vals, d_offs, M, K, outs["parent_b"])}
    t = timed(kinds, args.steps, args.graph_launches, dev)
    return {"part": "unchanged", "mix": mix, "B": B, "M": M, "new_us": t["new"], "parent_us": [t["parent_a"], t["parent_b"]],
            "parent_spread_us": abs(t["parent_a"] - t["parent_b"]), "new_minus_parent_us": [t["new"] - t["parent_a"], t["new"] - t["parent_b"]],
            "same_results": same(outs["new"], outs["parent_a"]) and same(outs["new"], outs["parent_b"])}


def part_index(mix, args, cfg, dev):
    B, M, K = args.B, args.M, args.max_spans
    chars, lens, d_vals, d_offs = corpus(mix, B, M, dev)
    d_chars, d_lens = torch.from_numpy(chars).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
    outs = {k: alloc_match(B, K, dev) for k in ("ragged_a", "ragged_b", "selected_ragged", "selected_padded")}
    sel = torch.arange(B, dtype=torch.int32, device=dev)
    kinds = {"ragged_a": lambda i: cfg.match_batch_ragged(d_vals, d_offs, max_spans=K, out=outs["ragged_a"]),
             "selected_ragged": lambda i: cfg.match_selected(d_vals, sel, offsets=d_offs, max_spans=K, out=outs["selected_ragged"]),
             "selected_padded": lambda i: cfg.match_selected(d_chars, sel, lens=d_lens, max_spans=K, out=outs["selected_padded"]),
             "ragged_b": lambda i: cfg.match_batch_ragged(d_vals, d_offs, max_spans=K, out=outs["ragged_b"])}
    t = timed(kinds, args.steps, args.graph_launches, dev)
    base = min(t["ragged_a"], t["ragged_b"])
    return {"part": "index", "mix": mix, "B": B, "M": M, "kernel": cfg.describe_match(B, layout=hra.LAYOUT_INPUT_SELECTED | hra.LAYOUT_INPUT_RAGGED),
            "ragged_us": [t["ragged_a"], t["ragged_b"]], "ragged_spread_us": abs(t["ragged_a"] - t["ragged_b"]), "selected_ragged_us": t["selected_ragged"],
            "selected_padded_us": t["selected_padded"], "selected_ragged_minus_ragged_us": t["selected_ragged"] - base,
            "selected_padded_minus_ragged_us": t["selected_padded"] - base,
            "same_results": same(outs["selected_ragged"], outs["ragged_a"]) and same(outs["selected_padded"], outs["ragged_a"])}


def part_ordered(mix, args, cfg, dev, B, directions=False):
    M, K = args.M, args.max_spans
    chars, lens, d_vals, d_offs = corpus(mix, B, M, dev)
    d_chars, d_lens = torch.from_numpy(chars).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
    cuts = [M * (j + 1) // 8 for j in range(8)]
    outs = {k: alloc_match(B, K, dev) for k in ("ragged", "padded", "ordered", "ascending", "descending")}
    rout = alloc_route(B, len(cuts), dev)

    def ordered(i):
        r = cfg.route(None, offsets=d_offs, bounds=cuts, out=rout)
        cfg.match_selected(d_vals, r.order, offsets=d_offs, max_spans=K, out=outs["ordered"])

    kinds = {"ragged": lambda i: cfg.match_batch_ragged(d_vals, d_offs, max_spans=K, out=outs["ragged"]),
             "padded": lambda i: cfg.match_batch(d_chars, d_lens, max_spans=K, out=outs["padded"]),
             "ordered": ordered}
    if directions:          # the order itself made once outside the graph: what the direction of the walk is worth
        asc = cfg.route(None, offsets=d_offs, bounds=cuts).order.clone()
        desc = torch.flip(asc, [0]).contiguous()
        kinds["ascending"] = lambda i: cfg.match_selected(d_vals, asc, offsets=d_offs, max_spans=K, out=outs["ascending"])
        kinds["descending"] = lambda i: cfg.match_selected(d_vals, desc, offsets=d_offs, max_spans=K, out=outs["descending"])
    t = timed(kinds, args.steps, args.graph_launches, dev)
    out = {"part": "ordered", "mix": mix, "B": B, "M": M, "cuts": cuts, "mean_len": float(lens.mean()), "ragged_us": t["ragged"], "padded_us": t["padded"],
           "route_plus_selected_us": t["ordered"], "ordered_over_ragged": t["ordered"] / t["ragged"], "ordered_over_padded": t["ordered"] / t["padded"],
           "ragged_over_padded": t["ragged"] / t["padded"], "same_results": all(same(outs[k], outs["ragged"]) for k in kinds)}
    if directions:
        out.update({"ascending_us": t["ascending"], "descending_us": t["descending"]})
    return out


def part_cascade(mix, args, screen, dev):
    B, M, K = args.B, args.M, args.max_spans
    four = configure(H4, M)
    _, _, d_vals, d_offs = corpus(mix, B, M, dev)
    sout, rout = alloc_match(B, K, dev), alloc_route(B, 1, dev)
    outs = {k: alloc_match(B, K, dev) for k in ("all", "survivors", "cascade")}
    st, _, _ = screen.match_batch_ragged(d_vals, d_offs, max_spans=K, out=sout)
    r = screen.route(st, offsets=d_offs, bounds=[M], require_accept=1, out=rout)
    kept = int(r.bucket_offsets.cpu()[1])          # (the 24 bytes a caller reads back between the two screens)
    sel = r.order[:kept].clone()

    def cascade(i):
        s, _, _ = screen.match_batch_ragged(d_vals, d_offs, max_spans=K, out=sout)
        screen.route(s, offsets=d_offs, bounds=[M], require_accept=1, out=rout)
        four.match_selected(d_vals, rout[0][:kept], offsets=d_offs, max_spans=K, out=outs["cascade"])

    kinds = {"all": lambda i: four.match_batch_ragged(d_vals, d_offs, max_spans=K, out=outs["all"]),
             "survivors": lambda i: four.match_selected(d_vals, sel, offsets=d_offs, max_spans=K, out=outs["survivors"]),
             "cascade": cascade}
    t = timed(kinds, args.steps, args.graph_launches, dev)
    idx = sel.cpu().numpy()
    return {"part": "cascade", "mix": mix, "B": B, "M": M, "kept": kept, "kept_share": kept / B,
            "launch": four.describe_match(max(kept, 1), layout=hra.LAYOUT_INPUT_SELECTED | hra.LAYOUT_INPUT_RAGGED)[:160],
            "via_rows_all_us": t["all"], "via_rows_survivors_us": t["survivors"], "screen_route_survivors_us": t["cascade"],
            "survivors_over_all": t["survivors"] / t["all"], "cascade_over_all": t["cascade"] / t["all"],
            "same_results": same(outs["survivors"], outs["all"], idx) and same(outs["cascade"], outs["all"], idx)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="unchanged,index,ordered,cascade")
    ap.add_argument("--parent-lib", default=None, help="another build of libhrx.so for the unchanged part (e.g. the parent commit's)")
    ap.add_argument("--mixes", default="all_M,uniform,skewed")
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--max-spans", type=int, default=16)
    ap.add_argument("--graph-launches", type=int, default=10, help="launches per captured graph (one timed interval)")
    ap.add_argument("--big", action="store_true", help="ordered: one more run at 4 B strings, with the order ascending and descending")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = configure([R1], args.M)
    parts, mixes = args.parts.split(","), args.mixes.split(",")
    for mix in mixes:
        if "unchanged" in parts and args.parent_lib:
            print(json.dumps(part_unchanged(mix, args, cfg, dev)), flush=True)
        if "index" in parts:
            print(json.dumps(part_index(mix, args, cfg, dev)), flush=True)
        if "ordered" in parts and mix != "all_M":
            print(json.dumps(part_ordered(mix, args, cfg, dev, args.B)), flush=True)
        if "cascade" in parts and mix != "all_M":
            print(json.dumps(part_cascade(mix, args, cfg, dev)), flush=True)
    if "ordered" in parts and args.big:
        print(json.dumps(part_ordered("uniform", args, cfg, dev, 4 * args.B, directions=True)), flush=True)


if __name__ == "__main__":
    main()
