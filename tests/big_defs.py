"""The cases of test_big_defs_cpu.py / test_big_defs_gpu.py: def sets with TWO synthetic 256-state DFAs (65537 transition rows each), alone and with a small
def before or between them, at tiny M — table size does not depend on M.  A string's run of lookup counts then needs four passes of lookup_counts_kernel,
a def begins inside a later pass, a def's bins touch three passes, an endpoint lookup straddles a pass border, and lookup_permute keeps two multi-chunk fill
lists per string side by side in its workspace.  properties() derives all of that from the context's own reports, and the CPU test asserts it, so that a
change to synth, to the run layout or to the planner cannot silently empty the matrix.  No device here."""
import functools

import numpy as np

import halo2_regex_amd as hra
from halo2_regex_amd import synth

BYTES = np.arange(256, dtype=np.uint8)
NAMES = ("trans", "start", "end")
TOO_LONG = 0xffffffff              # misses of a string without rows (include/hrx.h LOOKUP COUNTS)
M_SMALL, M_COUNTS = 19, (19, 64)


def big_def(seed):
    return synth.random_dfa(256, seed=seed, alphabet=BYTES, n_substr_pairs=200)


def small_def():
    """a few dozen states, total over the byte alphabet: noise keeps status 0 in it"""
    return synth.random_dfa(36, seed=7, alphabet=BYTES, n_substr_pairs=60, total=True)


@functools.lru_cache(maxsize=None)
def def_texts(name):
    """[(allstr_text, substr_text)] of a def set"""
    return {"big-big": lambda: [big_def(2), big_def(3)],
            "big-small-big": lambda: [big_def(2), small_def(), big_def(3)],
            "small-big-big": lambda: [small_def(), big_def(2), big_def(3)]}[name]()


SETS = ("big-big", "big-small-big", "small-big-big")


def configure(name, M, device):
    return hra.RegexVerifyConfig.configure(M, [hra.RegexDefs(hra.AllstrRegexDef(a), [hra.SubstrRegexDef(s)]) for a, s in def_texts(name)], device=device)


_refs = {}


def lookup_ref(oracle, name):
    """the LookupRef of a def set, built once (two dicts of 65537 rows)"""
    from lookup_ref import LookupRef
    from oracle_lib import OracleDefs
    if name not in _refs:
        _refs[name] = LookupRef(OracleDefs(oracle, [(a.encode(), [s.encode()]) for a, s in def_texts(name)]))
    return _refs[name]


def lens_of(M):
    return np.array([0, 1, 7, M - 1, M, M + 1, M, M - 1], np.uint32)


LONG = 5                           # the string of lens_of() without rows


def batch(M, seed=1):
    """8 strings of byte noise: lengths 0, 1, 7, M - 1, M, M + 1 (no rows), M, M - 1.  Every def is total, so every string with rows has status 0 in every def"""
    lens = lens_of(M)
    chars, _ = synth.noise(len(lens), M + 1, seed=seed, alphabet=BYTES)
    for b, n in enumerate(lens):
        chars[b, n:] = 0
    return np.ascontiguousarray(chars), lens


def pass_of(w, pass_words):
    return int(w) // pass_words


def properties(cfg, B):
    """what the matrix depends on, from the context's own reports: a dict"""
    lay, W = cfg.lookup_layout(), cfg.lookup_words()
    G, passes = cfg.lookup_group(B)
    pw = -(-W // passes)
    pw = (pw + 3) // 4 * 4                                  # a pass's range of a run: a multiple of 4 words (csrc/hrx_lookup.hpp plan_lookup)
    first = [l["trans"].start for l in lay]
    last = [l["end"].stop - 1 for l in lay]
    T = max(sl.stop - sl.start for l in lay for sl in l.values())
    plan = cfg.lookup_permute_plan(B, T)
    multi_chunk = [(3 * d + k, l[n]) for d, l in enumerate(lay) for k, n in enumerate(NAMES) if l[n].stop - l[n].start > plan["chunk_rows"]]
    big = [(col, sl) for col, sl in multi_chunk if sl.stop - sl.start == T]
    return dict(W=W, G=G, passes=passes, pass_words=pw, T=T, plan=plan, big=big, multi_chunk=multi_chunk,
                begins_mid_pass=[d for d in range(len(lay)) if pass_of(first[d], pw) > 0 and first[d] % pw != 0],
                touches_three=[d for d in range(len(lay)) if pass_of(last[d], pw) - pass_of(first[d], pw) >= 2],
                ranges_apart=[d for d, l in enumerate(lay) if len({pass_of(l["trans"].start, pw), pass_of(l["start"].start, pw), pass_of(l["end"].stop - 1, pw)}) == 3],
                straddling_endpoint=[(d, n) for d, l in enumerate(lay) for n in ("start", "end") if pass_of(l[n].start, pw) != pass_of(l[n].stop - 1, pw)],
                workspace=cfg.lookup_permute_workspace_bytes(B, T))


def fill_list(m):
    """the table rows S' places behind the first positions of A': every row no input hits, in order (row 0 too where m[0] == 0) — the numpy construction's own"""
    return np.nonzero(np.asarray(m) == 0)[0]


# ---- the tamper matrix of the counts tests ------------------------------------------------------------------------------------------------------
BITS = {"state": 1, "sid": 1 << 16, "se": 1 << 24, "ee": 1 << 25}


def tamper_rounds(M, mid_def):
    """rounds of {string: (kind, row, def)}, one mutation per string: a state, an id, a start and an end flag, each in def 0 and in the def that begins
    mid-pass, at row 0, a middle row and row M - 2 — on the strings of lens_of(M) that have those rows enabled (n >= M - 1; the string of 7 characters takes
    rows 0 and 3)"""
    full = [3, 4, 6, 7]
    combos = [(kind, row, d) for kind in BITS for d in (0, mid_def) for row in (0, M // 2, M - 2)]
    rounds, at = [], 0
    while at < len(combos):
        take = combos[at:at + len(full)]
        rnd = {b: c for b, c in zip(full, take)}
        kind, row, d = take[0]
        rnd[2] = (kind, 3 if row else 0, mid_def - d)      # (the other def of the pair)
        rounds.append(rnd)
        at += len(full)
    return rounds


# ---- hand-made counts for permute ---------------------------------------------------------------------------------------------------------------
def hand_made(cfg, n_rows):
    """(names, counts (4, W) uint32, overflow words): three patterns in BOTH big transition lookups of each string, a different one in each, (0, 2, 0, ...) in
    the endpoint lookups; the fourth string's second big lookup holds one too many beside sound lookups"""
    p = properties(cfg, 4)
    (c0, s0), (c1, s1) = p["big"][0], p["big"][-1]
    T = s0.stop - s0.start
    assert T == s1.stop - s1.start and c0 != c1 and n_rows >= T

    def nearly_all():
        m = np.zeros(T, np.uint32)
        m[40000], m[7] = T - 5, 3
        return m

    def every_other():
        m = np.zeros(T, np.uint32)
        m[0:T:2] = 1
        return m

    def all_but_row_0():
        m = np.ones(T, np.uint32)
        m[0] = 0
        return m

    pats = [nearly_all, every_other, all_but_row_0]
    W = cfg.lookup_words()
    counts = np.zeros((4, W), np.uint32)
    for l in cfg.lookup_layout():
        for n in ("start", "end"):
            counts[:, l[n].start + 1] = 2
    names = []
    for i in range(3):
        a, b = pats[i], pats[(i + 1) % 3]
        counts[i, s0], counts[i, s1] = a(), b()
        names.append(a.__name__ + " | " + b.__name__)
    counts[3, s0] = every_other()
    counts[3, s1] = all_but_row_0()
    counts[3, s1.start + 12345] += n_rows - (T - 1) + 1        # the sum is n_rows + 1
    names.append("every_other | one too many")
    over = np.array([0, 0, 0, 1 << c1], np.uint32)
    return names, counts, over
