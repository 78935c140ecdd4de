"""ROUTE (include/hrx.h) measured the way tools/ragged_bench.py and tools/extract_bench.py measure: HIP events around a captured graph of K launches of one
kind, the kinds taking turns, medians over --steps intervals; every result is checked against numpy after the timed region.  Three parts, one JSON line each:

  route     graph(match + route) - graph(match) on a ragged corpus: the three route launches beside the match launch they follow
  staging   hrx_ragged_to_position_major_device on full-length ragged strings: this build's <ragged, no index> instantiation, the same entry point of another
            build of the library (--parent-lib PATH, loaded beside this one; timed twice, so that its spread between two runs of itself is on the line) and
            the indexed form with sel = arange(B)
  e2e       per length mix (uniform, skewed): match, then either stage everything and witness it at M (the route a caller has today), or route into
            --bounds, gather each bucket and witness it at its own bound; the ratio of the two (whole, and with the match launch both begin with taken
            off) beside the ratio the written bytes predict
            (sum_j |bucket_j| * (4 D + 2) * bounds[j] against B * (4 D + 2) * M; the accept share of the planted corpus is on the line)

  python tools/route_bench.py [--parts route,staging,e2e] [--parent-lib PATH] [--B 65536] [--M 1024] [--bounds 64,256,1024] [--steps 20]
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/route_bench.py --steps 2      (a run of its own: the kernels' times)
"""
import argparse
import ctypes as C
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
from ragged_bench import lengths, timed  # noqa: E402

R1 = ["regex1_test_lookup.txt", ["substr1_test_lookup.txt"]]


def corpus(mix, B, M, dev):
    """regex1-planted strings cut to the mix's lengths -> (chars, lens, d_values, d_offsets)"""
    chars, _ = synth.regex1_planted(B, M, seed=0, stride=M)
    lens = lengths(mix, B, M, np.random.default_rng(0))
    chars[np.arange(M)[None, :] >= lens.astype(np.int64)[:, None]] = 0
    values, offsets = hra.pack_strings([chars[b, :lens[b]].tobytes() for b in range(B)])
    return chars, lens, torch.from_numpy(values).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)


def expect_route(status, n, bounds, require_accept):
    bounds = np.asarray(bounds, np.int64)
    keep = ((status & np.uint64(0xff)) == 0) & (((status >> np.uint64(8)) & np.uint64(require_accept)) == np.uint64(require_accept)) & (n <= bounds[-1])
    bins = np.where(keep, np.searchsorted(bounds, n, side="left"), len(bounds))
    return np.argsort(bins, kind="stable").astype(np.uint32), np.concatenate((np.zeros(1, np.uint64), np.cumsum(np.bincount(bins, minlength=len(bounds) + 1), dtype=np.uint64)))


def route_same(r, status, n, bounds, require_accept):
    want = expect_route(status.cpu().numpy().view(np.uint64), n, bounds, require_accept)
    return bool(np.array_equal(r.order.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(r.bucket_offsets.cpu().numpy().view(np.uint64), want[1]))


def alloc_route(B, n_buckets, dev):
    return (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(n_buckets + 2, dtype=torch.int64, device=dev),
            torch.empty(hra.route_workspace_bytes(B) // 8, dtype=torch.int64, device=dev))


def alloc_match(B, K, dev):
    return torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, K), dtype=torch.int64, device=dev)


def part_route(args, cfg, dev):
    B, M, K = args.B, args.M, args.max_spans
    _, lens, d_vals, d_offs = corpus("uniform", B, M, dev)
    mout, rout = alloc_match(B, K, dev), alloc_route(B, len(args.bounds), dev)
    match = lambda i: cfg.match_batch_ragged(d_vals, d_offs, max_spans=K, out=mout)

    def both(i):
        st, _, _ = match(i)
        return cfg.route(st, offsets=d_offs, bounds=args.bounds, require_accept=1, out=rout)

    t = timed({"match": match, "match_route": both}, args.steps, args.graph_launches, dev)
    r = both(0)
    torch.cuda.synchronize()
    added = t["match_route"] - t["match"]
    sizes = np.diff(r.bucket_offsets.cpu().numpy()).tolist()
    return {"part": "route", "B": B, "M": M, "bounds": args.bounds, "require_accept": 1, "mix": "uniform", "match": cfg.describe_match(B, layout=hra.LAYOUT_INPUT_RAGGED),
            "match_us": t["match"], "match_route_us": t["match_route"], "route_us": added, "route_over_match": added / t["match"], "bucket_sizes": sizes,
            "same_as_numpy": route_same(r, mout[0], lens.astype(np.int64), args.bounds, 1)}


class OtherLib:
    """another build of libhrx.so beside the package's, bound by hand: only what hrx_ragged_to_position_major_device needs (a build from before ROUTE lacks
    the symbols the package binds at import, so HRX_LIB_PATH cannot load it)"""

    def __init__(self, path, names, device):
        self.lib = lib = C.CDLL(path)
        vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
        for name, (res, argt) in {"hrx_defs_create": (i, [C.POINTER(vp)]), "hrx_defs_push_allstr_file": (i, [vp, C.c_char_p]),
                                  "hrx_defs_push_substr_file": (i, [vp, C.c_char_p]), "hrx_defs_finalize": (i, [vp]), "hrx_ctx_create": (i, [vp, i, C.POINTER(vp)]),
                                  "hrx_ragged_to_position_major_device": (i, [vp, vp, vp, sz, sz, vp, vp, vp])}.items():
            f = getattr(lib, name)
            f.restype, f.argtypes = res, argt
        self.defs, self.ctx = vp(), vp()
        ok = lambda rc: (_ for _ in ()).throw(RuntimeError("%s: rc %d" % (path, rc))) if rc else None
        ok(lib.hrx_defs_create(C.byref(self.defs)))
        for a, subs in names:
            ok(lib.hrx_defs_push_allstr_file(self.defs, os.path.join(DFA_DIR, a).encode()))
            for s in subs:
                ok(lib.hrx_defs_push_substr_file(self.defs, os.path.join(DFA_DIR, s).encode()))
        ok(lib.hrx_defs_finalize(self.defs))
        ok(lib.hrx_ctx_create(self.defs, device, C.byref(self.ctx)))          # (kept for the life of the process)

    def ragged_to_position_major(self, values, offsets, stride, out):
        rc = self.lib.hrx_ragged_to_position_major_device(self.ctx, values.data_ptr(), offsets.data_ptr(), offsets.numel() - 1, stride, out[0].data_ptr(),
                                                          out[1].data_ptr(), torch.cuda.current_stream(values.device).cuda_stream)
        assert rc == 0, rc


def part_staging(args, cfg, dev):
    B, M = args.B, args.M
    _, lens, d_vals, d_offs = corpus("all_M", B, M, dev)
    stride = -(-M // 16) * 16
    bufs = {k: (torch.zeros(B * stride, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)) for k in ("new", "indexed", "parent_a", "parent_b")}
    sel = torch.arange(B, dtype=torch.int32, device=dev)
    kinds = {"new": lambda i: cfg.ragged_to_position_major(d_vals, d_offs, stride=stride, out=bufs["new"]),
             "indexed": lambda i: cfg.gather_to_position_major(d_vals, sel, stride, offsets=d_offs, out=bufs["indexed"])}
    if args.parent_lib:
        other = OtherLib(args.parent_lib, [R1], 0)
        kinds["parent_a"] = lambda i: other.ragged_to_position_major(d_vals, d_offs, stride, bufs["parent_a"])
        kinds["parent_b"] = lambda i: other.ragged_to_position_major(d_vals, d_offs, stride, bufs["parent_b"])
    t = timed(kinds, args.steps, args.graph_launches, dev)
    torch.cuda.synchronize()
    same = all(torch.equal(bufs[k][0], bufs["new"][0]) and torch.equal(bufs[k][1], bufs["new"][1]) for k in kinds)
    want = torch.from_numpy(lens.astype(np.int32)).to(dev)
    out = {"part": "staging", "B": B, "M": M, "stride": stride, "mix": "all_M", "no_index_us": t["new"], "indexed_us": t["indexed"],
           "indexed_over_no_index": t["indexed"] / t["new"], "same_bytes": bool(same and torch.equal(bufs["new"][1], want))}
    if args.parent_lib:
        out.update({"parent_us": [t["parent_a"], t["parent_b"]], "parent_spread_us": abs(t["parent_a"] - t["parent_b"]),
                    "no_index_minus_parent_us": t["new"] - min(t["parent_a"], t["parent_b"])})
    return out


def part_e2e(mix, args, cfg, dev):
    B, M, K, bounds = args.B, args.M, args.max_spans, args.bounds
    D = cfg.num_defs
    chars, lens, d_vals, d_offs = corpus(mix, B, M, dev)
    stride = -(-M // 16) * 16
    mout, rout = alloc_match(B, K, dev), alloc_route(B, len(bounds), dev)
    # once, eagerly: the bucket sizes (the (n_buckets + 2) * 8 bytes a caller reads back), then every buffer at its size
    st, _, _ = cfg.match_batch_ragged(d_vals, d_offs, max_spans=K, out=mout)
    r = cfg.route(st, offsets=d_offs, bounds=bounds, require_accept=1, out=rout)
    bo = r.bucket_offsets.cpu().numpy()
    same = route_same(r, st, lens.astype(np.int64), bounds, 1)
    all_in = (torch.empty(B * stride, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    all_out = cfg.alloc_outputs_position_major(B, dev)
    per = []
    for j, Mj in enumerate(bounds):
        n = int(bo[j + 1] - bo[j])
        sj = -(-Mj // 16) * 16
        with cfg.circuit_size(Mj):
            per.append((n, sj, r.order[int(bo[j]):int(bo[j + 1])], (torch.empty(n * sj, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)),
                        cfg.alloc_outputs_position_major(n, dev) if n else None))

    def everything(i):
        cfg.match_batch_ragged(d_vals, d_offs, max_spans=K, out=mout)
        cfg.ragged_to_position_major(d_vals, d_offs, stride=stride, out=all_in)
        cfg.witness_batch_position_major(all_in[0], all_in[1], out=all_out, chars_pm_stride=stride)

    def routed(i):
        s, _, _ = cfg.match_batch_ragged(d_vals, d_offs, max_spans=K, out=mout)
        cfg.route(s, offsets=d_offs, bounds=bounds, require_accept=1, out=rout)
        for (n, sj, sel, gin, wout), Mj in zip(per, bounds):
            if n == 0:
                continue
            cfg.gather_to_position_major(d_vals, sel, sj, offsets=d_offs, out=gin)
            with cfg.circuit_size(Mj):
                cfg.witness_batch_position_major(gin[0], gin[1], out=wout, chars_pm_stride=sj)

    match = lambda i: cfg.match_batch_ragged(d_vals, d_offs, max_spans=K, out=mout)
    t = timed({"match": match, "everything": everything, "routed": routed}, args.steps, args.graph_launches, dev)
    torch.cuda.synchronize()
    # the routed witness of every kept string = its rows in the witness of everything (status words of the two; rows are compared by tests/test_route_gpu.py)
    st_all = all_out[2].cpu().numpy()
    order = r.order.cpu().numpy()
    for (n, sj, sel, gin, wout), Mj, j in zip(per, bounds, range(len(bounds))):
        if n:
            idx = order[int(bo[j]):int(bo[j + 1])]
            short = lens[idx] < Mj                   # (n == M: the status of the two sizes differs by design)
            same = same and bool(np.array_equal(wout[2].cpu().numpy()[short], st_all[idx][short])) and bool(np.array_equal(gin[1].cpu().numpy(), lens[idx].astype(np.int32)))
    sizes = np.diff(bo).tolist()
    predicted = sum(n * Mj for n, Mj in zip(sizes, bounds)) / float(B * M)
    return {"part": "e2e", "mix": mix, "B": B, "M": M, "D": D, "bounds": bounds, "require_accept": 1, "mean_len": float(lens.mean()), "bucket_sizes": sizes,
            "accept_share": float(sum(sizes[:-1])) / B, "match_us": t["match"], "everything_us": t["everything"], "routed_us": t["routed"], "measured_ratio": t["routed"] / t["everything"],
            "measured_ratio_after_match": (t["routed"] - t["match"]) / (t["everything"] - t["match"]),
            "predicted_ratio_written_bytes": predicted, "same_results": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="route,staging,e2e")
    ap.add_argument("--parent-lib", default=None, help="another build of libhrx.so for the staging part (e.g. the parent commit's)")
    ap.add_argument("--mixes", default="uniform,skewed")
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--bounds", default="64,256,1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--max-spans", type=int, default=16)
    ap.add_argument("--graph-launches", type=int, default=10, help="launches per captured graph (one timed interval)")
    args = ap.parse_args()
    args.bounds = [int(x) for x in args.bounds.split(",")]
    dev = torch.device("cuda", 0)
    defs = [hra.RegexDefs(hra.AllstrRegexDef.read_from_text(os.path.join(DFA_DIR, a)), [hra.SubstrRegexDef.read_from_text(os.path.join(DFA_DIR, s)) for s in subs])
            for a, subs in [R1]]
    cfg = hra.RegexVerifyConfig.configure(args.M, defs, device=0)
    parts = args.parts.split(",")
    if "route" in parts:
        print(json.dumps(part_route(args, cfg, dev)), flush=True)
    if "staging" in parts:
        print(json.dumps(part_staging(args, cfg, dev)), flush=True)
    if "e2e" in parts:
        for mix in args.mixes.split(","):
            print(json.dumps(part_e2e(mix, args, cfg, dev)), flush=True)


if __name__ == "__main__":
    main()
