"""The launch planner's choices over a sweep of configs, layouts, shapes and settings, as the texts of hrx_describe_launch / hrx_describe_match
(host only: no device is needed to plan).  tests/test_plan_golden_cpu.py replays the sweep against the built library and compares it with
tests/golden/launch_plans.json; this file defines the sweep and records the fixture.

Recording is done ONCE, against a libhrx.so built from the commit the refactored code descends from, never from the code under test:

    git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/halo2_regex_amd/csrc
    HRX_LIB_PATH=/tmp/parent/halo2_regex_amd/csrc/libhrx.so python tests/golden/record_launch_plans.py --commit <parent commit>

    ... --dump DIR     every text of the sweep in full, one file per config (diff a failing line against the parent's dump)

    ... --note NAME --parent-dump DIR     where the launch and the describe text of the parent DISAGREED and the text now follows the launch, the
                                          line keeps the parent's digest and gets a note: the digest of the corrected text, taken from the loaded (new)
                                          library after every differing text passed the note's rule against the parent's dump (NOTES below)

A LINE of the sweep is one (what, config, layout, M, num_cus, setting) over the whole B list of that num_cus.  The fixture holds a digest per line
and the full text at SAMPLES of the B list, texts stored once in a table.  An answer that is an error is recorded as "ERR <code>: <message>"."""
import argparse
import base64
import ctypes as C
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(HERE, "launch_plans.json")
DFA_DIR = os.path.join(HERE, "dfa")

PLANES, RAGGED, SELECTED = 4, 8, 16           # LAYOUT_RECORD_PLANES, LAYOUT_INPUT_RAGGED, LAYOUT_INPUT_SELECTED
LAUNCH_LAYOUTS = (0, 1, 3, 1 | PLANES, 3 | PLANES)
MATCH_LAYOUTS = (0, 2, RAGGED, SELECTED, SELECTED | RAGGED)
MS = (8, 64, 1000, 1001, 1024, 2048, 4096, 32768)
SETTING_MS = (64, 1001, 4096)
CUS = (256, 255, 64, 1)
VIA_ROWS = 1 << 32                            # kDbgMatchViaRows
RECORDED_ROWS = 21                            # rows of the variant matrix when the fixture was recorded: their settings are lines of the sweep

# every bit of kDbgForceMask (csrc/hrx_kernel.hpp)
FORCE_BITS = (0x10000, 0x20000, 0x40000, 0x80000, 0x200000, 0x400000, 0x2000, 0x8000, 0x2000000, 0x4000000, 0x8000000, 0x40000000, 0x100000,
              0x800, 0x1000, 0x10000000, 0x20000000, 0x80, 0x80000000)


def b_list(cus):
    """B at the planner's thresholds for a device of `cus` CUs"""
    bs = [1, 63, 64, 65]
    for k in (1, 2, 4, 8):
        bs += [64 * k * cus - 64, 64 * k * cus, 64 * k * cus + 64]
    for per4 in (7, 6):                       # the chunked launch stops above 7/4 (two defs) and 6/4 (three) groups per CU
        g = cus * per4 // 4
        bs += [64 * (g - 1), 64 * g, 64 * (g + 1)]
    bs += [65536, 65537, 70000, 1 << 20]
    return sorted({b for b in bs if b > 0})


def samples(cus):
    """the B values whose text the fixture holds in full: a small batch, the chunked / def-parallel range, a full chip with dynamic groups"""
    return (64, 64 * cus, 1 << 20)


def _files(names):
    rd = lambda f: open(os.path.join(DFA_DIR, f)).read()
    return [(rd(a), [rd(s) for s in subs]) for a, subs in names]


def configs():
    """name -> [(allstr_text, [substr_text, ...])]: what the tests already build (test_abi._defs, test_parity_gpu's configs of the stored DFA files,
    synth.random_dfa, a fuzz_defs shape of the variant matrix)"""
    import fuzz_defs as fd
    from halo2_regex_amd import synth
    R1, R2, R3 = (["regex%d_test_lookup.txt" % k, ["substr%d_test_lookup.txt" % k]] for k in (1, 2, 3))
    HDR = [["header_from_lookup.txt", ["header_from_substr0.txt"]], ["header_to_lookup.txt", ["header_to_substr0.txt"]],
           ["header_subject_lookup.txt", ["header_subject_substr%d.txt" % k for k in range(3)]]]
    EX = ["ex_allstr.txt", ["ex_substr_id1.txt"]]
    nosub = lambda cfg: [[a, []] for a, _ in cfg]
    allb = np.arange(256, dtype=np.uint8)
    big = lambda *a, **kw: [(lambda t: (t[0], [t[1]]))(synth.random_dfa(*a, **kw))]
    many = big(40, seed=3, alphabet=allb)                      # a def of more than 32 byte classes: no CLASS-WIDE table for a config that holds it
    fuzz = lambda seed, shape: [(a, subs) for a, subs, _ in fd.make_case(seed, shape).defs_t]
    c = {
        "pair1": _files([R1]),
        "wide2": _files([R1, R2]),
        "wide3": _files([R1, R2, R3]),
        "big256": big(256, seed=2, alphabet=allb, n_substr_pairs=200),                     # BYTE and HALF images
        "big256_ids": fuzz(0, fd.Shape(1, 1, "big", ids=("ids_64", "ids_65"))),            # substring ids past the BYTE slot
        "nohalf300": big(300, seed=2),                                                     # the 4-byte table does not fit LDS, no HALF image
        # a table that leaves LDS for the one-wave kernel's waves of 16 strings but not of 64: string-major odd row counts of big batches fit no launch (HRX_ERR_BOUNDS)
        "tight140": big(140, seed=2),
        "cw4": _files([R1, R2, R3, HDR[0]]),
        "cw5": _files([R3, HDR[2], R1, HDR[1], R2]),
        "cw6": _files(HDR + [R1, R2, R3]),
        "cw8": _files([R1, R2, R3] + HDR + [R1, R2]),
        "nocw4": _files([R1, R2, R3]) + many,
        "nocw5": _files([R1, R2, R3, HDR[0]]) + many,
        "nocw6": _files([R1, R2, R3, HDR[0], HDR[1]]) + many,
        "nocw7": _files([R1, R2, R3] + HDR) + many,
        "nocw12": _files([R1, R2, R3] + HDR + nosub([R1, R2, R3] + HDR[:2])) + many,      # four groups of three: the most the last pass merges itself
        "d13": _files([R1, R2, R3] + HDR + nosub([R1, R2, R3] + HDR) + [EX]),
        "d16": _files(HDR + nosub([R1, R2, R3]) + [R1, R2, R3] + nosub(HDR + [R1, R2, R3]) + [R1]),
    }
    return c


def settings():
    """name -> dict(flags, mpc, option): the default; every single bit of kDbgForceMask; the rows of the variant matrix; the combiner-wave option;
    HRX_MP_COMBINE; the match entry's "via rows" bit"""
    from test_variants_gpu import ROWS
    s = {"bit_%x" % b: dict(flags=b) for b in FORCE_BITS}
    for r in ROWS[:RECORDED_ROWS]:
        s["row_" + r["id"]] = dict(flags=r["flags"], mpc=bool(r.get("mp_combine")), option=r.get("option"))
    # (the matrix's later rows reach their variants by shape — row counts, def counts, batch sizes — under settings the recorded rows already hold: no lines of their own)
    held = {(st["flags"], st["mpc"], st["option"]) for name, st in s.items() if name.startswith("row_")}
    assert all((r["flags"], bool(r.get("mp_combine")), r.get("option")) in held for r in ROWS[RECORDED_ROWS:])
    for v in (0, 1, 2):
        s["combiner_wave_%d" % v] = dict(flags=0, option=(1, v))
    for v in (0, 1):
        s["mp_combine_%d" % v] = dict(flags=0, mpc_env=str(v))
    s["via_rows"] = dict(flags=VIA_ROWS)
    return s


def sweep():
    """the lines, in the fixture's order: (what, config, layout, M, num_cus, setting name)"""
    out = []
    names = list(configs_cached())
    for cfg in names:
        for what, layouts in (("launch", LAUNCH_LAYOUTS), ("match", MATCH_LAYOUTS)):
            for lay in layouts:
                for M in MS:
                    for cus in CUS:
                        out.append((what, cfg, lay, M, cus, "default"))
    for cfg in names:
        for name, st in settings().items():
            # launch: string-major and position-major; the planes form where the setting holds a context option (the combiner wave follows the planes).
            # match: the bits a match plan reads, padded; the ragged form where the setting changes how a via-rows call ends
            launch = (0, 3, 3 | PLANES) if st.get("option") else (0, 3)
            match = () if name.startswith("row_") or name.startswith("combiner_") else (0, RAGGED) if name == "via_rows" or name.startswith("mp_") else (0,)
            for what, layouts in (("launch", launch), ("match", match)):
                for lay in layouts:
                    for M in SETTING_MS:
                        out.append((what, cfg, lay, M, 256, name))
    return out


_CONFIGS = None


def configs_cached():
    global _CONFIGS
    if _CONFIGS is None:
        _CONFIGS = configs()
    return _CONFIGS


class Planner:
    """describe_* of one config under the sweep's settings: through hrx_describe_* (the environment a context created now would read), or — where the
    setting holds a context option — through a host-only context made under that environment"""

    def __init__(self, hra, defs_t):
        self.hra = hra
        defs = [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(t) for t in subs]) for a, subs in defs_t]
        self.cfg = hra.RegexVerifyConfig.configure(64, defs, device=None)
        self.ctxs = {}
        self.buf = C.create_string_buffer(8192)

    def __del__(self):
        for ctx in self.ctxs.values():
            self.hra.lib.hrx_ctx_destroy(ctx)

    @staticmethod
    def _with_env(setting, fn):
        env = {"HRX_DEBUG_FLAGS": str(setting.get("flags", 0))}
        if setting.get("mpc"):
            env["HRX_MP_COMBINE"] = "1"
        if "mpc_env" in setting:
            env["HRX_MP_COMBINE"] = setting["mpc_env"]
        saved = {k: os.environ.get(k) for k in ("HRX_DEBUG_FLAGS", "HRX_MP_COMBINE")}
        for k in saved:
            os.environ.pop(k, None)
        os.environ.update(env)
        try:
            return fn()
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v

    def _ctx(self, sname, setting):
        if sname not in self.ctxs:
            ctx = C.c_void_p()
            assert self.hra.lib.hrx_ctx_create(self.cfg._defs.h, self.hra.HRX_DEVICE_NONE, C.byref(ctx)) == 0
            assert self.hra.lib.hrx_ctx_set_option(ctx, *setting["option"]) == 0
            self.ctxs[sname] = ctx
        return self.ctxs[sname]

    def texts(self, sname, setting, what, layout, M, cus, bs):
        lib, buf = self.hra.lib, self.buf

        def run():
            ctx = self._ctx(sname, setting) if setting.get("option") and cus == 256 else None
            out = []
            for B in bs:
                if ctx:
                    rc = (lib.hrx_ctx_describe_launch if what == "launch" else lib.hrx_ctx_describe_match)(ctx, layout, B, M, buf, 8192)
                else:
                    rc = (lib.hrx_describe_launch if what == "launch" else lib.hrx_describe_match)(self.cfg._defs.h, layout, B, M, cus, buf, 8192)
                out.append(buf.value.decode() if rc == 0 else "ERR %d: %s" % (rc, lib.hrx_last_error().decode("utf-8", "replace")))
            return out
        return self._with_env(setting, run)


def pack(obj):
    """samples (per line, the indices of its sample texts) and the text table: JSON, deflated, base64 — the texts repeat most of their words and would
    not fit the repository's limit for a fixture otherwise; --dump shows them in full"""
    return base64.b64encode(zlib.compress(json.dumps(obj, separators=(",", ":")).encode(), 9)).decode()


def unpack(payload):
    return json.loads(zlib.decompress(base64.b64decode(payload)))


def load_fixture(path=FIXTURE):
    fx = json.load(open(path))
    fx.update(unpack(fx.pop("payload")))
    n = len(fx["digests"]) // fx["lines"]
    fx["digests"] = [fx["digests"][i * n:(i + 1) * n] for i in range(fx["lines"])]
    fx["noted"] = {}        # line index -> (note name, digest of the corrected texts)
    for name, note in fx.get("notes", {}).items():
        for item in note["lines"].split():
            i, d = item.split(":")
            fx["noted"][int(i)] = (name, d)
    return fx


def _chunked_group_pass(parent, new):
    """the same text (of a witness call, or of a match call that goes via rows) but for 'chunked=' in passes of a multi-pass config, and their geometry"""
    head, sep, _ = parent.partition("multi-pass, ")
    return bool(sep) and new.startswith(head + sep) and "chunked=" in parent and "chunked=" not in new and \
        parent.count("[defs ") == new.count("[defs ") and parent.split("] ")[-1] == new.split("] ")[-1]


# name -> (reason, rule(parent_text, new_text) -> the difference is the one the note is about)
NOTES = {
    "chunked_group_pass": (
        "The parent's describe text planned a pass of a multi-pass config (a group of three defs) like a launch of its own and so named it 'chunked=' for few "
        "long strings; its launch_batch never chunked a pass (the planner saw the summary / merge arguments there, and a chunked launch of a group was an "
        "error).  Launch and text now read one route plan: a pass is described unchunked, as it always ran.",
        _chunked_group_pass),
}


def key_of(line):
    return "%s %s layout=%d M=%d cus=%d %s" % line


def digest(texts):
    """of one line's texts: 18 bits, three characters (a changed plan changes whole families of lines; one line slipping through by chance does not matter)"""
    return base64.b64encode(hashlib.sha256("\n".join(texts).encode()).digest()[:3]).decode()[:3]


def run_sweep(hra, on_line):
    """on_line(index, line, bs, texts) for every line of the sweep"""
    sets = dict(settings(), default=dict(flags=0))
    planners = {}
    for i, line in enumerate(sweep()):
        what, cfg, lay, M, cus, sname = line
        pl = planners.get(cfg)
        if pl is None:
            pl = planners[cfg] = Planner(hra, configs_cached()[cfg])
        bs = b_list(cus)
        on_line(i, line, bs, pl.texts(sname, sets[sname], what, lay, M, cus, bs))


def add_note(hra, args):
    parent = {}
    for name in os.listdir(args.parent_dump):
        for row in open(os.path.join(args.parent_dump, name)):
            k, t = row.rstrip("\n").split(" | ", 1)
            parent[k] = t
    fx = json.load(open(args.out))
    n = len(fx["digests"]) // fx["lines"]
    rule, noted = NOTES[args.note][1], {}

    def on_line(i, line, bs, texts):
        if digest(texts) == fx["digests"][i * n:(i + 1) * n]:
            return
        for B, t in zip(bs, texts):
            was = parent["%s B=%d" % (key_of(line), B)]
            assert was == t or rule(was, t), "not what the note is about: %s B=%d\n  parent: %s\n  now:    %s" % (key_of(line), B, was, t)
        noted[i] = digest(texts)
    run_sweep(hra, on_line)
    fx.setdefault("notes", {})[args.note] = {"reason": NOTES[args.note][0], "lines": " ".join("%d:%s" % kv for kv in sorted(noted.items()))}
    with open(args.out, "w") as f:
        json.dump(fx, f, indent=0)
    print("%d noted lines (%s), %d bytes -> %s" % (len(noted), args.note, os.path.getsize(args.out), args.out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", help="hash of the commit the loaded library was built from (stored in the fixture)")
    ap.add_argument("--dump", metavar="DIR", help="write every text in full to DIR instead of the fixture")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--note", choices=sorted(NOTES), help="add the note's corrected digests to the fixture, from the loaded library")
    ap.add_argument("--parent-dump", metavar="DIR", help="with --note: the parent's --dump, which every differing text is checked against")
    args = ap.parse_args()
    import halo2_regex_amd as hra
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        files = {}

        def dump(i, line, bs, texts):
            f = files.get(line[1]) or files.setdefault(line[1], open(os.path.join(args.dump, line[1] + ".txt"), "w"))
            for B, t in zip(bs, texts):
                f.write("%s B=%d | %s\n" % (key_of(line), B, t))
        run_sweep(hra, dump)
        for f in files.values():
            f.close()
        return
    if args.note:
        return add_note(hra, args)
    if not args.commit:
        ap.error("--commit: the fixture names the commit it was recorded from")
    table, index, digests, sample_refs = [], {}, [], []

    def rec(i, line, bs, texts):
        digests.append(digest(texts))
        refs = []
        for B in samples(line[4]):
            t = texts[bs.index(B)]
            if t not in index:
                index[t] = len(table)
                table.append(t)
            refs.append(index[t])
        sample_refs.append(refs)
    run_sweep(hra, rec)
    with open(args.out, "w") as f:
        json.dump({"recorded_from_commit": args.commit, "library": "libhrx.so of that commit, loaded through HRX_LIB_PATH",
                   "lines": len(digests), "digests": "".join(digests), "payload": pack({"samples": sample_refs, "texts": table})}, f, indent=0)
    print("%d lines, %d texts, %d bytes -> %s" % (len(digests), len(table), os.path.getsize(args.out), args.out))


if __name__ == "__main__":
    main()
