"""Seeded generator of regex definitions and batches in the reference's text formats, with the edge cases where the table builders
(csrc/hrx_defs.cpp) and the kernels can be subtly wrong.  Plain module (no GPU, no pytest): tests/test_variants_gpu.py runs its
cases through every forced kernel variant, tests/test_variants_cpu.py through the host walk and checks what the seeds cover.

A case is a function of (seed, Shape) alone.  Each case records in `edges` which edge cases it holds:

definitions
  unused_below_L      largest_state_val above the highest state used, and unused state numbers below it
  first_nonzero       first_state_val != 0
  accept_is_first     accepted_state_val == first_state_val
  accept_unreachable  an accepted state no transition leads to
  endpoint_above_L    substring start / end states above largest_state_val (dropped by the table builder)
  pair_untaken        substring pairs the DFA never takes (states above largest_state_val among them)
  ids_62 .. ids_65    one def whose substring ids reach 62 .. 65 (a BYTE-table slot holds 6 bits of id)
  ids_sum_255         the defs' last substring ids sum to exactly 255 (the u8 limit of hrx_defs_finalize)
  big_total, big_partial, partial_255   150..256-state DFAs; 255 partial states fill all 256 BYTE rows
  few_classes         a total DFA over 2..4 bytes (the PAIR table's byte classes)
strings
  undef_0, undef_n-1, undef_M-1       an undefined transition at position 0, at the string's last byte, at row M-1
  undef_odd, undef_even               ... at an odd / even position (the two halves of a pair step)
  undef_3, undef_4, undef_7, undef_8, undef_63, undef_64   ... on each side of the quad, octet and 64-row borders
  byte_0, byte_127, byte_128, byte_255                     these bytes inside a string (the WIDE table has no column >= 128)
  len_0, len_1, len_M-1, len_M, len_M+1                    string lengths
"""
import dataclasses

import numpy as np

M_SMALL = (1, 2, 3, 5, 7, 8, 9, 31, 33, 100, 257)
M_16 = (16, 32, 48, 64, 80, 128, 144, 256, 320, 512)
M_8X = (8, 24, 40, 56, 72, 136, 264, 328)      # M % 16 == 8: below the transposer's 32-row tile, one octet on each side of its border, a partial last tile
BATCHES = (1, 63, 64, 65, 129)
PM_BLOCK = 65536          # strings per block of the position-major layouts (include/hrx.h)
UNDEF_EDGES = ("undef_0", "undef_n-1", "undef_M-1", "undef_odd", "undef_even", "undef_3", "undef_4", "undef_7", "undef_8", "undef_63", "undef_64")
BYTE_EDGES = ("byte_0", "byte_127", "byte_128", "byte_255")
LEN_EDGES = ("len_0", "len_1", "len_M-1", "len_M", "len_M+1")
DEF_EDGES = ("unused_below_L", "first_nonzero", "accept_is_first", "accept_unreachable", "endpoint_above_L", "pair_untaken")
ALL_EDGES = DEF_EDGES + ("ids_62", "ids_63", "ids_64", "ids_65", "ids_sum_255", "big_total", "big_partial", "partial_255", "few_classes") + UNDEF_EDGES + BYTE_EDGES + LEN_EDGES


@dataclasses.dataclass(frozen=True)
class Shape:
    """What a kernel variant can take.  states: 'small' (3..60 states), 'big' (150..256: HALF / BYTE tables), 'pair' (a total DFA over 2..4 bytes).
    m: 'any' (small and odd M too), 'm16' (multiples of 16), 'm8' (M % 8 == 0), 'm8x' (M % 16 == 8), 'odd8' (M % 8 != 0).  ids: substring-id edges the variant can
    take ('ids_62' .. 'ids_65', 'ids_sum_255').  ascii: every def's bytes below 128 (the WIDE table)."""
    d_lo: int = 1
    d_hi: int = 1
    states: str = "small"
    m: str = "any"
    ids: tuple = ()
    ascii: bool = False
    big_kinds: tuple = ("big_total", "big_partial", "partial_255")
    m_max: int = 1 << 30
    s_max: int = 60       # small DFAs: at most this many states
    min_batch: int = 0    # the batch repeated until it holds at least this many strings (variants that only large batches reach)


@dataclasses.dataclass
class Case:
    seed: int
    defs_t: list          # [(allstr_text, [substr_text, ...], alphabet)]
    M: int
    B: int
    stride: int           # a multiple of 16, > M
    chars: np.ndarray     # (B, stride) uint8
    lens: np.ndarray      # (B,) uint32
    edges: set
    plants: list          # [(string, position, edge)]: an undefined transition of def 0 planted there

    @property
    def D(self):
        return len(self.defs_t)


def _alphabet(rng, shape, lo=2, hi=24):
    top = 128 if shape.ascii else 256
    return np.sort(rng.choice(np.arange(1, top), size=int(rng.integers(lo, hi)), replace=False)).astype(np.uint8)


def _def_text(rng, S, alpha, dens, opts, n_subs, edges, few_pairs=False, silent=False, marker=None):
    """One definition: S used states, renumbered into 0..L (with gaps: unused_below_L), hubs 0..3 of the used ones; n_subs substring definitions."""
    L = S - 1
    names = np.arange(S)
    if "unused_below_L" in opts:
        L = S - 1 + int(rng.integers(2, 6))
        names = np.sort(rng.choice(np.arange(L), size=S, replace=False))      # L itself (and some below it) never used
        edges.add("unused_below_L")
    first = int(rng.integers(0, S))
    if "first_nonzero" in opts:
        first = int(rng.integers(1, S)) if S > 1 else 0
        if names[first] != 0:
            edges.add("first_nonzero")
    trans = {}
    for st in range(S):
        for ch in alpha:
            if dens >= 1.0 or rng.random() < dens:
                nx = int(rng.integers(0, S)) if rng.random() < 0.5 else int(rng.integers(0, min(S, 4)))
                trans[(st, int(ch))] = nx
    if marker is not None:      # the marker byte leads every state into a state of its own, flagged as a substring start: def 1 flags exactly where it is planted
        for st in range(S):
            trans[(st, marker)] = S
        for ch in alpha:
            trans[(S, int(ch))] = int(rng.integers(0, min(S, 4)))
        S += 1
        names = np.append(names, L + 1)
        L += 1
    if dens < 1.0:      # a partial DFA keeps one defined byte per state: the walks go on
        for st in range(S):
            if not any((st, int(ch)) in trans for ch in alpha):
                trans[(st, int(alpha[int(rng.integers(0, len(alpha)))]))] = int(rng.integers(0, S))
    acc_name = int(names[int(rng.integers(0, min(S, 4)))])
    if "accept_is_first" in opts:
        acc_name = int(names[first])
        edges.add("accept_is_first")
    if "accept_unreachable" in opts:
        if L == S - 1:
            L = S      # one state number no transition uses
        unused = sorted(set(range(L + 1)) - set(int(x) for x in names))
        if unused:
            acc_name = unused[int(rng.integers(0, len(unused)))]
            edges.add("accept_unreachable")
    lines = [str(int(names[first])), str(acc_name), str(L)]
    pairs = set()
    for (st, ch), nx in sorted(trans.items()):
        lines.append("%d %d %d" % (names[st], names[nx], ch))
        pairs.add((int(names[st]), int(names[nx])))
    pairs = sorted(pairs)
    subs = []
    hubs = set(int(x) for x in names[:4])
    rare = [p for p in pairs if p[0] not in hubs and p[1] not in hubs] or pairs
    used = set()
    for j in range(n_subs):
        if marker is not None and j == 0:
            z = int(names[-1])
            mp = sorted({(int(names[st]), z) for st in range(S - 1)})
            subs.append("\n".join(["8", "0", "99", " ".join(str(a) for a, _ in mp) + " ", "%d " % z] + ["%d %d" % p for p in mp]) + "\n")
            continue
        if few_pairs:       # one pair between states off the hubs: flags beside def 0's are rare, and overlap (status 2) only now and then
            pick = [rare[int(rng.integers(0, len(rare)))]]
            a, b = (L + 1, L + 1) if silent else pick[0]      # silent: ids only, the endpoints are dropped (no flags)
            subs.append("\n".join(["8", "0", "99", "%d " % a, "%d " % b, "%d %d" % pick[0]]) + "\n")
            continue
        if n_subs > 3 and j > 0:        # the id edges: one pair of its own per substring definition (the BYTE table's tag hash takes a few hundred pairs at most)
            free = [p for p in pairs if p not in used] or pairs
            pick = [free[int(rng.integers(0, len(free)))]]
        else:
            k = min(len(pairs), int(rng.integers(4, 40)) if n_subs <= 3 else int(rng.integers(2, 8)))
            pick = [pairs[i] for i in rng.choice(len(pairs), size=k, replace=False)]
        used.update(pick)
        starts = sorted({a for a, _ in pick[: max(1, len(pick) // 3)]})
        ends = sorted({b for _, b in pick[len(pick) // 2:]}) or [pick[0][1]]
        if "endpoint_above_L" in opts and j == 0:
            starts.append(L + 1 + int(rng.integers(0, 3)))
            ends.append(L + 1 + int(rng.integers(3, 6)))
            edges.add("endpoint_above_L")
        if "pair_untaken" in opts and j == 0:
            taken = set(pairs)
            for a in range(L + 3):
                if (a, 0) not in taken:
                    pick.append((a, 0))
                    break
            pick.append((L + 2, int(names[0])))
            edges.add("pair_untaken")
        subs.append("\n".join(["8", "0", "99", " ".join(map(str, starts)) + " ", " ".join(map(str, ends)) + " "] +
                              ["%d %d" % p for p in sorted(set(pick))]) + "\n")
    walk = {(int(names[st]), ch): int(names[nx]) for (st, ch), nx in trans.items()}
    return "\n".join(lines) + "\n", subs, alpha, (int(names[first]), acc_name, walk)


def _sub_counts(rng, D, shape, edges, seed):
    """substring definitions per def: 1..3, or one of the id edges the shape takes (chosen by the seed)"""
    counts = [int(rng.integers(1, 4)) for _ in range(D)]
    if shape.ids and seed % 2 == 0:
        pick = shape.ids[(seed // 2) % len(shape.ids)]
        if pick == "ids_sum_255" and D >= 2:
            # last id of def d = n_0 + .. + n_d: sum over d of (D - d) n_d = 255
            counts = [1] * D
            rest = 255 - sum((D - d) * counts[d] for d in range(D - 1))
            counts[D - 1] = rest
            edges.add("ids_sum_255")
        elif pick.startswith("ids_6"):
            counts[0] = int(pick[4:])          # def 0's ids are 1..n
            edges.add(pick)
    return counts


def make_case(seed, shape):
    rng = np.random.default_rng(77000 + seed)
    edges = set()
    D = shape.d_lo + seed % (shape.d_hi - shape.d_lo + 1)       # consecutive seeds walk the whole range
    counts = _sub_counts(rng, D, shape, edges, seed)
    opts = {DEF_EDGES[(seed + k) % len(DEF_EDGES)] for k in range(2)}      # two of the definition edges per seed, in turn
    defs_t, walks = [], []
    shared = _alphabet(rng, shape)
    marker = int(shared[-1]) if D >= 2 and len(shared) >= 3 else None     # planted only where status 2 is wanted
    big_multi = shape.states == "big" and D > 1      # other defs beside the big one: all of them over the big def's bytes and the shared ones (no draw more or less)
    for d in range(D):
        dens = 1.0
        if shape.states == "big" and d == 0:
            kind = shape.big_kinds[seed % len(shape.big_kinds)]
            if kind == "big_total":
                S, dens, alpha = int(rng.integers(150, 257)), 1.0, _alphabet(rng, shape, 20, 60)
            elif kind == "big_partial":
                S, dens, alpha = int(rng.integers(150, 255)), 0.9, _alphabet(rng, shape, 20, 60)
            else:       # 255 states, no gaps in the numbering: with the dead row, all 256 BYTE rows
                S, dens, alpha = 255, 0.9, _alphabet(rng, shape, 20, 60)
                opts = opts - {"unused_below_L", "accept_unreachable"}
            if "unused_below_L" in opts or "accept_unreachable" in opts:      # (unused state numbers: stay within 256 rows)
                S = min(S, 250)
            if big_multi:
                alpha = np.union1d(alpha, shared).astype(np.uint8)
            if kind != "partial_255":
                edges.add(kind)
        elif shape.states == "pair" and d == 0:
            S, alpha = int(rng.integers(3, 40)), _alphabet(rng, shape, 2, 5)
            edges.add("few_classes")
        else:
            S = int(rng.integers(3, shape.s_max + 1))
            if d == 0:
                alpha = shared if D > 1 or rng.random() < 0.8 else _alphabet(rng, shape, 2, 40)
                dens = float(rng.choice([1.0, 1.0, 0.97, 0.9]))
            else:       # total over the shared bytes: the walks of def 0 decide how a string ends, the other defs flag rows beside it
                alpha = defs_t[0][2] if big_multi else shared
        a_t, subs, al, walk = _def_text(rng, S, alpha, dens, opts if d == 0 else set(), counts[d], edges, few_pairs=d > 0, silent=d > 0, marker=marker if d == 1 else None)
        if shape.states == "big" and d == 0 and kind == "partial_255" and a_t.split("\n", 3)[2] == "254" and len({ln.split()[0] for ln in a_t.split("\n")[3:] if ln}) == 255:
            edges.add("partial_255")
        defs_t.append((a_t, subs, al))
        walks.append(walk)
    # ---- the batch
    if shape.m == "m16":
        pool_m = [m for m in M_16 if m <= shape.m_max]
    elif shape.m == "m8":
        pool_m = [m for m in M_16 + (8,) if m <= shape.m_max]
    elif shape.m == "m8x":
        pool_m = [m for m in M_8X if m <= shape.m_max]
    elif shape.m == "odd8":
        pool_m = [m for m in M_SMALL + (100, 260) if m % 8 and m <= shape.m_max]
    else:
        pool_m = [m for m in M_SMALL + M_16 if m <= shape.m_max]
    M = int(pool_m[seed % len(pool_m)]) if seed % 3 == 0 else int(rng.choice(pool_m))
    if seed % 6 == 4:
        M = max(pool_m)       # room for every planted position
    B = int(BATCHES[seed % len(BATCHES)])
    stride = (M + 1 + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))      # > M: the strings of length M + 1 are readable
    first, acc, walk = walks[0]
    a0 = defs_t[0][2]
    common = a0
    for _, _, a in defs_t[1:]:
        common = np.intersect1d(common, a)
    union = np.unique(np.concatenate([a for _, _, a in defs_t]))
    outside = np.setdiff1d(np.arange(1, 256), union)
    by_state = {}
    for (st, ch), nx in walk.items():
        by_state.setdefault(st, []).append(ch)
    common_set = set(int(c) for c in common)
    chars = np.zeros((B, stride), np.uint8)
    lens = np.zeros(B, np.uint32)
    plants = []
    len_cycle = [("len_0", 0), ("len_1", 1), ("len_M-1", M - 1), ("len_M", M), ("len_M+1", M + 1)]
    for b in range(B):
        # lengths: the edges in turn on every seventh string, else mostly long
        if b % 7 == 3:
            name, n = len_cycle[(b // 7 + seed) % len(len_cycle)]
            if 0 <= n <= M + 1:
                edges.add(name)
        else:
            n = M if rng.random() < 0.4 else int(rng.integers(0, M + 1))
        if B == 1:
            name, n = len_cycle[seed % len(len_cycle)] if seed % 4 == 3 else ("len_M", M)
            if n < 0:
                n = M
            edges.add(name)
        # a walk of def 0 over defined bytes (the ones every def knows where it can); it ends in the accepted state on some strings
        st, row = first, np.empty(stride, np.uint8)
        seen_acc = -1
        for i in range(stride):
            opts_b = by_state.get(st, [])
            if marker is not None:
                opts_b = [c for c in opts_b if c != marker] or opts_b
            pref = [c for c in opts_b if c in common_set]
            c = (pref if pref and rng.random() < 0.9 else opts_b or [int(union[0])])
            c = int(c[int(rng.integers(0, len(c)))])
            row[i] = c
            st = walk.get((st, c), st)
            if st == acc and seen_acc < 0 and 0 < i + 1 <= M:
                seen_acc = i + 1
        if seen_acc > 0 and b % 5 == 1 and n != M + 1:
            n = seen_acc
        chars[b] = row
        lens[b] = n
    # the marker byte (def 1 flags a start there: two defs flagging one row is status 2) in a few strings
    if marker is not None:
        for b in range(10, B, 11):
            n = int(lens[b])
            if 0 < n <= M:
                for p in rng.integers(0, n, size=4):
                    chars[b, int(p)] = marker
    # undefined transitions of def 0, planted: every edge in turn over the strings that are long enough
    k = seed
    for b in range(B):
        if not (b % 6 == 5 or B == 1 and seed % 4 == 1):
            continue
        n = int(lens[b])
        for _ in range(len(UNDEF_EDGES)):
            edge = UNDEF_EDGES[k % len(UNDEF_EDGES)]
            k += 1
            p = {"undef_0": 0, "undef_n-1": n - 1, "undef_M-1": M - 1, "undef_odd": 1 + 2 * int(rng.integers(0, max(1, M // 2))),
                 "undef_even": 2 * int(rng.integers(0, max(1, (M + 1) // 2))), "undef_3": 3, "undef_4": 4, "undef_7": 7, "undef_8": 8,
                 "undef_63": 63, "undef_64": 64}[edge]
            if 0 <= p < M and not (edge == "undef_odd" and p % 2 == 0) and not (edge == "undef_even" and p % 2):
                break
        else:
            continue
        if n > M:
            continue
        if n <= p:
            n = p + 1
            lens[b] = n
        st = first
        for i in range(p):
            st = walk.get((st, int(chars[b, i])), st)
        holes = [int(c) for c in a0 if (st, int(c)) not in walk]
        if holes and rng.random() < 0.7:
            chars[b, p] = holes[int(rng.integers(0, len(holes)))]
        elif len(outside):
            chars[b, p] = int(outside[int(rng.integers(0, len(outside)))])
        else:
            continue
        plants.append((b, p, edge))
        edges.add(edge)
    # the bytes 0, 127, 128, 255 inside some strings
    for j, b in enumerate(range(2, B, 9) if B > 1 else ([0] if seed % 4 == 2 else [])):
        n = int(lens[b])
        if 0 < n <= M and b not in {q for q, _, _ in plants}:
            v = (0, 127, 128, 255)[(j + seed) % 4]
            chars[b, int(rng.integers(0, n))] = v
            edges.add("byte_%d" % v)
    if shape.min_batch > B:      # (the plants keep their indices: they lie in the first copy)
        r = -(-shape.min_batch // B)
        chars, lens, B = np.tile(chars, (r, 1)), np.tile(lens, r), B * r
    return Case(seed, defs_t, M, B, stride, chars, lens, edges, plants)


def extra_seeds(base):
    """HRX_FUZZ_EXTRA="a:b,c:d" adds these seed ranges to a row's fixed seeds (a soak run)"""
    import os
    seeds = list(base)
    for part in os.environ.get("HRX_FUZZ_EXTRA", "").split(","):
        if ":" in part:
            a, b = part.split(":")
            seeds += [x for x in range(int(a), int(b)) if x not in seeds]
    return seeds
