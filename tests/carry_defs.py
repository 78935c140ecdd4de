"""Deterministic scenarios for the reveal mask's carries (src/lib.rs:593-764, oracle/hrx_oracle.c:427-455): "lever" definitions in the reference's
text formats whose start / end flags and substring ids land on exactly the rows a test chooses, and strings that keep a range of rows pending over
hundreds to tens of thousands of event-free rows before an event (or the string's end) confirms it or takes it back.  Plain module (no GPU, no
pytest), like tests/fuzz_defs.py: tests/test_carry_gpu.py runs the batches through every kernel, tests/test_carry_cpu.py checks that they are what
they claim and runs them through the host walk.

The lever DFA (ours, made for these tests): states 0..3, every byte defined in every state.

    byte   next state                                   role
    f      3 if q == 3 else 0                           filler, substring id 0
    s      1                                            out of state 0: a START (forward set, backward reset); out of 2 / 3: the id changes, no flag
    r      1 if q == 1 else (3 if q == 3 else 0)        continues a run
    e      2                                            after x: an END without a start (backward set, forward reset one row later)
    x      3                                            arms an end-only e
    y      0

One substring definition: every transition into state 1 or 2, start states {0}, end states {2}.  Forms:

  second=True   states 4, 5 and the bytes t (-> 4), u (stays in 4), d (-> 5) with a second substring definition (every transition into 4 or 5, start
                states {0, 2}, end states {5}): the id changes A -> B without a flag (`s r t`), with a start (`f t`), and `x e t` puts A's end flag and
                B's start flag on one row (index of t).
  D = 2 .. 12   def k has six lever bytes of its own (LEVERS[k]); the bytes of the other defs are filler to it.  ST / EN / SID are sums over the
                defs, so `x e` of def 1 confirms a range def 0's `s` opened, and def 1's `s` takes it back.  The byte BOTH is `s` to every def:
                out of state 0 two defs flag one row (status 2).
  pad=n         n more states (HALF / BYTE tables want 150 .. 256): the byte p walks through them in a ring, every other byte acts in them as in
                state 0; transitions out of them carry no id.  A few p in the filler make the walk visit the high state numbers.
  classes=n     n more bytes (0x80 ..), each into a state of its own: a def of 6 + n byte classes (> 32: the class-table kernels' wide form).
  reduced=True  the bytes f, s, e, x only (a PAIR table takes 2 .. 4 byte classes).  s out of state 1 continues a run, so every one-def scenario
                stays; what drops out is everything that needs a second substring definition or a second def, and nothing else.

A scenario is a function of (M, a, b): the row `a` where a range opens (the `s`) and the row `b` where it is resolved (the `e` of `x e`, the second
`s`, or the string's length).  The reference never assigns an end flag to row M (lib.rs:501-519 stops at M - 1), so an `e` on row M - 1 confirms
nothing: confirmed ranges are resolved at M - 2 at the latest, and `e` at M - 1 is one more way for a range to be taken back."""
import numpy as np

import fuzz_defs as fd

LEVERS = [b"fsrexy", b"FSREXY", b"!\"#$%&", b"'()*+,", b"-./012", b"345678", b"9:;<=>", b"?@ABCD"]
LEVERS += [bytes(range(0xB0 + 6 * j, 0xB6 + 6 * j)) for j in range(4)]      # defs 8 .. 11: 0xB0 .. 0xC7, above every CLASS0 + j (which end below 0xA8)
BOTH = ord("b")
UNDEF = ord("~")             # no def has a transition for it
PADB = ord("p")
SECOND = b"tud"
CLASS0 = 0x80
TILE = 64


def lever_def(k=0, D=1, second=False, pad=0, classes=0, reduced=False, filler=()):
    """def k of D: (allstr_text, [substr_text, ...], alphabet); filler: further bytes that act like f (other defs' bytes of their own)"""
    f, s, r, e, x, y = LEVERS[k]
    core = 6 if second else 4
    S = core + pad + classes
    trans = {}

    def like0(q):
        return q if q == 3 else 0
    others = [c for j in range(D) if j != k for c in LEVERS[j]] + list(filler)
    for q in range(S):
        trans[(q, f)] = like0(q)
        trans[(q, s)] = 1
        trans[(q, e)] = 2
        trans[(q, x)] = 3
        if reduced:
            continue
        trans[(q, r)] = 1 if q == 1 else like0(q)
        trans[(q, y)] = 0
        trans[(q, BOTH)] = 1
        for c in others:
            trans[(q, c)] = like0(q)
        if second:
            t, u, d = SECOND
            trans[(q, t)] = 4
            trans[(q, u)] = 4 if q == 4 else like0(q)
            trans[(q, d)] = 5
        if pad:
            trans[(q, PADB)] = core + (q - core + 1) % pad if core <= q < core + pad else core
        for j in range(classes):
            trans[(q, CLASS0 + j)] = core + pad + j
    lines = ["0", "2", str(S - 1)] + ["%d %d %d" % (q, nx, c) for (q, c), nx in sorted(trans.items())]
    tagged_a = [(q, z) for z in (1, 2) for q in range(core)]
    subs = ["\n".join(["8", "0", "99", "0 ", "2 "] + ["%d %d" % p for p in tagged_a]) + "\n"]
    if second:
        tagged_b = [(q, z) for z in (4, 5) for q in range(core)]
        subs.append("\n".join(["8", "0", "99", "0 2 ", "5 "] + ["%d %d" % p for p in tagged_b]) + "\n")
    alpha = np.array(sorted({c for _, c in trans}), np.uint8)
    return "\n".join(lines) + "\n", subs, alpha


def lever_defs(D=1, second=False, pad=0, classes=0, reduced=False):
    """D lever defs; the forms apply to def 0 (second, pad, reduced) and to the last def (classes); what is a byte of its own to one def is filler to the others"""
    out = []
    for k in range(D):
        sec, pd, cl = second and k == 0, pad if k == 0 else 0, classes if k == D - 1 else 0
        fill = ([] if sec or not second else list(SECOND)) + ([] if pd or not pad else [PADB]) + ([] if cl else [CLASS0 + j for j in range(classes)])
        out.append(lever_def(k, D, second=sec, pad=pd, classes=cl, reduced=reduced, filler=fill))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------------
# scenario strings
class _Str:
    def __init__(self, n, reduced=False):
        self.v = np.full(n, LEVERS[0][0], np.uint8)      # def 0's f is filler to every def
        self.reduced = reduced

    def put(self, pos, letters, k=0):
        """letters of "fsrexy" as def k's bytes, from row pos"""
        for i, ch in enumerate(letters):
            if self.reduced and ch == "r":
                ch = "s"
            if 0 <= pos + i < len(self.v):
                self.v[pos + i] = LEVERS[k]["fsrexy".index(ch)]

    def raw(self, pos, byte):
        if 0 <= pos < len(self.v):
            self.v[pos] = byte


# every scenario: f(M, a, b, ko, kr, reduced) -> (bytes, expected status code, ranges) with ranges = [(first row, resolving row, "confirmed" | "taken_back")];
# ko: the def whose s opens the range, kr: the def that resolves it.  None where (a, b) leaves no room.
def sc_confirmed(M, a, b, ko=0, kr=0, reduced=False):
    """s at a ... x e at b - 1, b: rows a .. b revealed, all but the two ends with substring id 0"""
    if not (0 <= a and a + 2 <= b <= M - 2):
        return None
    s = _Str(min(M, b + 4), reduced=reduced)
    s.put(a, "s", ko)
    s.put(b - 1, "xe", kr)
    return s.v, 0, [(a, b, "confirmed")]


def sc_second_start(M, a, b, ko=0, kr=0, reduced=False):
    """s at a ... s at b out of state 0 (backward reset): rows a .. b - 1 taken back; the range the second s opens is taken back by the string's end"""
    if not (0 <= a and a + 2 <= b <= M - 1):
        return None
    s = _Str(min(M, b + 3), reduced=reduced)
    s.put(a, "s", ko)
    s.put(b, "s", kr)
    return s.v, 0, [(a, b, "taken_back")]


def sc_string_end(M, a, b, ko=0, kr=0, reduced=False):
    """s at a, the string ends at n = b < M"""
    if not (0 <= a < b < M):
        return None
    s = _Str(b, reduced=reduced)
    s.put(a, "s", ko)
    return s.v, 0, [(a, b, "taken_back")]


def sc_reach_m(M, a, b=None, ko=0, kr=0, reduced=False):
    """s at a, n == M: nothing behind row M - 1 (tile_is_exact's second clause)"""
    if not 0 <= a < M:
        return None
    s = _Str(M, reduced=reduced)
    s.put(a, "s", ko)
    return s.v, 0, [(a, M, "taken_back")]


def sc_end_at_last_row(M, a, b=None, ko=0, kr=0, reduced=False):
    """s at a, x e on rows M - 2, M - 1 of a full-length string: the reference assigns no end flag to row M, the range is taken back"""
    if not 0 <= a <= M - 3:
        return None
    s = _Str(M, reduced=reduced)
    s.put(a, "s", ko)
    s.put(M - 2, "xe", kr)
    return s.v, 0, [(a, M, "taken_back")]


def sc_end_only(M, a, b, ko=0, kr=0, reduced=False):
    """x e at b - 1, b with nothing in front: end_mask = 1 on rows 0 .. b, start_mask = 0: nothing revealed"""
    if not 1 <= b <= M - 2:
        return None
    s = _Str(min(M, b + 2), reduced=reduced)
    s.put(b - 1, "xe", kr)
    return s.v, 0, []


def sc_run(M, a, b, ko=0, kr=0, reduced=False):
    """a well-formed run s r r ... r e over rows a .. b (every row has the id)"""
    if not (0 <= a and a + 1 <= b <= M - 2):
        return None
    s = _Str(min(M, b + 2), reduced=reduced)
    s.put(a, "s" + "r" * (b - a - 1) + "e", ko)
    return s.v, 0, [(a, b, "confirmed")]


def sc_two_ranges(M, a, b, ko=0, kr=0, reduced=False, first_confirmed=True):
    """two ranges in one string, split at the middle of (a, b): one confirmed, the other taken back"""
    mid = (a + b) // 2
    if not (0 <= a and a + 3 <= mid and mid + 4 <= b <= M - 2):
        return None
    s = _Str(min(M, b + 5), reduced=reduced)
    s.put(a, "s", ko)
    if first_confirmed:      # s .. x e | s .. (string end)
        s.put(mid - 1, "xe", kr)
        s.put(mid + 2, "s", ko)
        s.v = s.v[:min(len(s.v), b)]
        return s.v, 0, [(a, mid, "confirmed"), (mid + 2, b, "taken_back")]
    s.put(mid, "s", kr)      # s .. | s .. x e
    s.put(b - 1, "xe", kr)
    return s.v, 0, [(a, mid, "taken_back"), (mid, b, "confirmed")]


def sc_islands(M, a, b, ko=0, kr=0, reduced=False, confirmed=True, every=37, count=None):
    """islands of tagged rows (x s r r: three rows with the id, no flag) inside a filler range, which is then confirmed or taken back"""
    if not (0 <= a and a + 12 <= b <= M - 2):
        return None
    s = _Str(min(M, b + 4), reduced=reduced)
    s.put(a, "s", ko)
    if count is not None:
        every = max(6, (b - a - 8) // count)
    p, k = a + 3, 0
    while p + 6 <= b - 2 and (count is None or k < count):
        s.put(p, "xsrr", ko)
        p += every
        k += 1
    if confirmed:
        s.put(b - 1, "xe", kr)
    else:
        s.put(b, "s", kr)
    return s.v, 0, [(a, b, "confirmed" if confirmed else "taken_back")]


def sc_over_cap(M, a, b, ko=0, kr=0, reduced=False, cap=4):
    """two short runs, then 3 * cap islands inside a range that is taken back at b (the run count goes from above the cap back below it), then one more run"""
    if not (8 <= a and a + 6 * 3 * cap + 12 <= b <= M - 8):
        return None
    s = _Str(min(M, b + 8), reduced=reduced)
    s.put(0, "sre", ko)
    s.put(4, "se", ko)
    v, _, _ = sc_islands(M, a, b, ko, kr, reduced, confirmed=False, count=3 * cap)
    s.v[a:b + 1] = v[a:b + 1]
    s.put(b + 1, "re", kr)      # the second start's own run: s r e, confirmed
    return s.v, 0, [(a, b, "taken_back")]


def sc_undefined(M, a, b, ko=0, kr=0, reduced=False):
    """an undefined byte at b inside the range a opened: status 1 (rows unspecified)"""
    if not (0 <= a < b <= M - 1):
        return None
    s = _Str(min(M, b + 6), reduced=reduced)
    s.put(a, "s", ko)
    s.raw(b, UNDEF)
    return s.v, 1, []


def sc_overlap(M, a, b, ko=0, kr=0, reduced=False):
    """the byte that is s to every def at b, behind the range a opened: two defs flag row b (status 2; D >= 2)"""
    if not (0 <= a and a + 2 <= b <= M - 1):
        return None
    s = _Str(min(M, b + 6), reduced=reduced)
    s.put(a, "s", ko)
    s.raw(b, BOTH)
    return s.v, 2, []


def sc_second_substr(M, a, b, variant=0):
    """def 0 with its second substring definition (D == 1, second=True): the range a opened is resolved at b by
    0: `x e t u d`  A's end flag and B's start flag on one row (confirms; B's run follows)      1: `x s r t u u` then x e: the id changes 0 -> A -> B -> 0 without a flag inside the range
    2: `d` out of state 0: B's start and end on one row (a start: takes the range back)"""
    t, u, d = SECOND
    if not (0 <= a and a + 10 <= b <= M - 8):
        return None
    s = _Str(min(M, b + 8))
    s.put(a, "s")
    if variant == 0:
        s.put(b - 1, "xe")
        for i, c in enumerate((t, u, u, d)):
            s.raw(b + 1 + i, c)
        return s.v, 0, [(a, b + 4, "confirmed")]      # (the set wins on the shared row: B's run t u u d is revealed with the range)
    if variant == 1:
        mid = (a + b) // 2
        s.put(mid, "xsr")
        for i, c in enumerate((t, u, u)):
            s.raw(mid + 3 + i, c)
        s.put(b - 1, "xe")
        return s.v, 0, [(a, b, "confirmed")]
    s.raw(b, d)
    return s.v, 0, [(a, b, "taken_back")]


def borders(M, chunk=0, n=None):
    """the rows where ranges open and are resolved: the quad / octet / tile-word / tile / forced-chunk / planner-chunk borders, every border of the launch's own
    chunks, the string ends; each with the row before and after it"""
    base = [0, 4, 8, 16, 32, 64, 256, 1024, 4096, M]
    if chunk:
        base += list(range(chunk, M, chunk))
    if n is not None:
        base.append(n)
    out = set()
    for p in base:
        out |= {p - 1, p, p + 1}
    return sorted(p for p in out if 0 <= p <= M)


def far(M, p):
    """a partner row for p at least M - 80 rows away where there is room, else as far as the string allows"""
    return M - 2 - (p % 5) if p < M // 2 else p % 7


class Batch:
    """chars (B, stride) u8, lens (B,) u32, want (B,) expected status code, ranges per string, names per string"""

    def __init__(self, M, defs_t):
        self.M, self.defs_t = M, defs_t
        self.rows, self.want, self.ranges, self.names = [], [], [], []

    def add(self, name, made):
        if made is None:
            return False
        v, code, ranges = made
        assert len(v) <= self.M
        self.rows.append(np.asarray(v, np.uint8))
        self.want.append(code)
        self.ranges.append(ranges)
        self.names.append(name)
        return True

    def case(self, min_batch=0, limit=None):
        """fd.Case: the scenario strings spread over the lanes, an empty and a full-length filler string after every sixth of them (so the fix loops
        of one wave have very different lengths)"""
        M = self.M
        idx = list(range(len(self.rows)))
        if limit is not None and len(idx) > limit:      # keep the longest ranges and every status
            key = lambda i: -max([abs(r[1] - r[0]) for r in self.ranges[i]] + [M + 1 if self.want[i] else 0])
            idx = sorted(sorted(idx, key=key)[:limit])
        rows, want, ranges, names = [], [], [], []
        for j, i in enumerate(idx):
            if j % 6 == 2:
                rows.append(np.zeros(0, np.uint8)); want.append(0); ranges.append([]); names.append("empty")
            if j % 6 == 5:
                rows.append(np.full(M, LEVERS[0][0], np.uint8)); want.append(0); ranges.append([]); names.append("filler")
            rows.append(self.rows[i]); want.append(self.want[i]); ranges.append(self.ranges[i]); names.append(self.names[i])
        B = len(rows)
        stride = (M + 1 + 15) // 16 * 16
        chars = np.zeros((B, stride), np.uint8)
        lens = np.zeros(B, np.uint32)
        for b, v in enumerate(rows):
            chars[b, :len(v)] = v
            lens[b] = len(v)
        if min_batch > B:
            r = -(-min_batch // B)
            chars, lens, B = np.tile(chars, (r, 1)), np.tile(lens, r), B * r
            want, ranges, names = want * r, ranges * r, names * r
        c = fd.Case(0, self.defs_t, M, B, stride, chars, lens, set(), [])
        c.want, c.ranges, c.names = np.array(want), ranges, names
        return c


def scenario_batch(M, D=1, second=False, pad=0, classes=0, reduced=False, chunk=0, min_batch=0, limit=None, cap=4, lean=False):
    """The batch for one launch: every border row opens a range and resolves one (the partner row far away), in every way a range can be resolved; the
    fixed scenarios; the multi-def and second-substring ones where the form has them.  lean: one opening and one resolved range per border instead of one
    per way of resolving it (the long-string launches, where a string costs 2^16 rows and more)."""
    defs_t = lever_defs(D, second=second, pad=pad, classes=classes, reduced=reduced)
    bt = Batch(M, defs_t)
    kw = dict(reduced=reduced)
    P = borders(M, chunk)
    resolvers = [("confirmed", sc_confirmed), ("second_start", sc_second_start), ("string_end", sc_string_end)]
    for i, p in enumerate(P):
        ko, kr = i % D, (i // 2) % D
        # a range opening at p, resolved far behind it (or as far as there is room); lean: in one way per border, the ways in turn
        done = False
        for j in range(3):
            if lean and done:
                break
            nm, fn = resolvers[(i + j) % 3]
            b = far(M, p) if p < M // 2 else min(M - 2 if fn is sc_confirmed else M - 1, p + 2 + j)
            done |= bt.add("%s open@%d" % (nm, p), fn(M, p, b, ko, kr, **kw))
        if not lean or not done or i % 4 == 0:
            bt.add("reach_m open@%d" % p, sc_reach_m(M, p, None, ko, kr, **kw))
        # a range resolved at p, opened far in front of it
        done = False
        for j in range(3):
            if lean and done:
                break
            nm, fn = resolvers[(i + j + 1) % 3]
            a = far(M, p) if p >= M // 2 else max(0, p - 2 - j)
            done |= bt.add("%s resolve@%d" % (nm, p), fn(M, a, p, ko, (kr + 1) % D, **kw))
        if not lean or i % 4 == 1:
            bt.add("end_only@%d" % p, sc_end_only(M, 0, p, ko, kr, **kw))
    a, b = 3, M - 5
    bt.add("fix_start_0", sc_second_start(M, 0, M - 3, **kw))
    bt.add("end_at_last_row", sc_end_at_last_row(M, 1, **kw))
    bt.add("run", sc_run(M, a, b, **kw))
    bt.add("run_tile", sc_run(M, 64, min(M - 2, 128), **kw))
    bt.add("two_ranges_ct", sc_two_ranges(M, a, b, first_confirmed=True, **kw))
    bt.add("two_ranges_tc", sc_two_ranges(M, a, b, first_confirmed=False, **kw))
    bt.add("islands_confirmed", sc_islands(M, a, b, confirmed=True, **kw))
    bt.add("islands_taken_back", sc_islands(M, a, b, confirmed=False, **kw))
    bt.add("over_cap", sc_over_cap(M, 9, b - 8, cap=cap, **kw))
    bt.add("over_cap_tile", sc_over_cap(M, 9, min(b - 8, 9 + 18 * cap + 12 + 64), cap=cap, **kw))
    bt.add("undefined", sc_undefined(M, a, M // 2 + 1, **kw))
    bt.add("undefined_last", sc_undefined(M, a, M - 1, **kw))
    if not reduced and pad:      # the walk visits the padded states: p runs inside a pending range
        for q in (1, pad - 1, pad + 3):
            made = sc_confirmed(M, a, b)
            if made and b - a > q + 20:
                made[0][a + 5:a + 5 + q] = PADB
                bt.add("pad_walk_%d" % q, made)
    if classes:
        made = sc_confirmed(M, a, b, D - 1, D - 1)
        if made:
            for j in range(classes):
                if a + 4 + 3 * j < b - 4:
                    made[0][a + 4 + 3 * j] = CLASS0 + j
            bt.add("class_walk", made)
    if D >= 2:
        bt.add("overlap", sc_overlap(M, a, b))
        bt.add("overlap_mid", sc_overlap(M, a, M // 2))
        for ko in range(D):
            kr = (ko + 1) % D
            bt.add("confirmed d%d->d%d" % (ko, kr), sc_confirmed(M, a + ko, b - kr, ko, kr))
            bt.add("second_start d%d->d%d" % (ko, kr), sc_second_start(M, a + ko, b - kr, ko, kr))
            bt.add("islands d%d->d%d" % (ko, kr), sc_islands(M, a + ko, b - kr, ko, kr, confirmed=ko % 2 == 0))
    if second:
        for v in range(3):
            bt.add("second_substr_%d" % v, sc_second_substr(M, a, b - 8, v))
            bt.add("second_substr_%d_tile" % v, sc_second_substr(M, 60, min(b - 8, 190 + v), v))
    return bt.case(min_batch=min_batch, limit=limit)


def all_repair_batch(M, B, D=1, chunk=256):
    """every chunk of every string is an item of the chunked launch's repair list (chunks x B of them, the list's capacity): s in front of row 3, a second start just
    behind the first chunk border (chunk 0 wrote its rows behind the s with end_mask = 1 and they are taken back), x e at M - 2 / M - 3 (every later chunk inherits
    start_mask = 1 where the launch assumed 0, and is revealed); islands in some strings"""
    bt = Batch(M, lever_defs(D))
    for i in range(B):
        ko, kr = i % D, (i // 2) % D
        a, a2, b = i % 3, chunk + 1 + i % 2, M - 2 - i % 2
        v, code, ranges = sc_islands(M, a2, b, kr, kr, every=chunk // 2 + 5) if i % 3 == 2 else sc_confirmed(M, a2, b, kr, kr)
        v[a] = LEVERS[ko][1]
        bt.add("all_repair", (v, code, [(a, a2, "taken_back")] + ranges))
    c = bt.case()
    keep = [i for i, nm in enumerate(c.names) if nm == "all_repair"]      # no empty / filler strings here
    c.chars, c.lens, c.want, c.B = c.chars[keep], c.lens[keep], c.want[keep], len(keep)
    c.ranges, c.names = [c.ranges[i] for i in keep], [c.names[i] for i in keep]
    return c


def no_repair_batch(M, B, D=1, chunk=256):
    """nothing crosses a chunk border: short runs and ranges inside the chunks, filler elsewhere"""
    bt = Batch(M, lever_defs(D))
    for i in range(B):
        s = _Str(M if i % 2 else M - 1 - i % 50)
        for c0 in range(0, M - chunk + 1, chunk):
            if (c0 // chunk + i) % 2 == 0:
                s.put(c0 + 3 + i % 40, "srrre", i % D)
            else:
                s.put(c0 + 5 + i % 30, "s", i % D)
                s.put(c0 + 100 + i % 60, "xe", (i + 1) % D)
        bt.add("no_repair", (s.v, 0, []))
    c = bt.case()
    keep = [i for i, nm in enumerate(c.names) if nm == "no_repair"]
    c.chars, c.lens, c.want, c.B = c.chars[keep], c.lens[keep], c.want[keep], len(keep)
    c.ranges, c.names = [c.ranges[i] for i in keep], [c.names[i] for i in keep]
    return c


def block_border_batch(M, D=1):
    """more than 65536 strings (two position-major blocks): short filler strings, and long confirmed / taken-back ranges in strings 65535 and 65536
    (and 65534 / 65537 the other way round)"""
    B = 65536 + 64
    bt = Batch(M, lever_defs(D))
    stride = (M + 1 + 15) // 16 * 16
    chars = np.zeros((B, stride), np.uint8)
    lens = (np.arange(B) % 7).astype(np.uint32)
    chars[:, :8] = LEVERS[0][0]
    want = np.zeros(B, np.int64)
    ranges, names = [[] for _ in range(B)], ["short"] * B
    plant = {65535: sc_confirmed(M, 1, M - 2), 65536: sc_second_start(M, 0, M - 1), 65534: sc_reach_m(M, 2), 65537: sc_islands(M, 3, M - 3),
             0: sc_confirmed(M, 0, M - 3), B - 1: sc_string_end(M, 1, M - 1), 63: sc_islands(M, 2, M - 4, confirmed=False), 65536 + 62: sc_run(M, 1, M - 2)}
    for b, (v, code, r) in plant.items():
        chars[b, :] = 0
        chars[b, :len(v)] = v
        lens[b], want[b], ranges[b], names[b] = len(v), code, r, "planted"
    c = fd.Case(0, bt.defs_t, M, B, stride, chars, lens, set(), [])
    c.want, c.ranges, c.names = want, ranges, names
    return c


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the reveal mask on the summed columns, vectorised (tests/test_carry_cpu.py holds the row-by-row transcription and checks the two against each other
# and against the oracle), the models of a kernel that left a carry out, and the range metric
def columns(o, text, M):
    """(SID (M,), ST (M + 1,), EN (M + 1,)) of one string from the oracle's match_substrs columns: sums over the defs; EN[i + 1] = end_enable[i]"""
    cols = o.match_substrs(bytes(text), M)
    sid = cols["substr_id"].sum(axis=0).astype(np.int64)
    st = np.concatenate((cols["start_enable"].sum(axis=0), [0])).astype(np.int64)
    en = np.concatenate(([0], cols["end_enable"].sum(axis=0))).astype(np.int64)
    return cols, sid, st, en


def _fill(ev, backward=False):
    """ev: 1 set, 0 reset, -1 nothing; the value of the last event at or before each index (after it, backward), 0 before the first"""
    if backward:
        return _fill(ev[::-1])[::-1]
    idx = np.where(ev >= 0, np.arange(len(ev)), -1)
    idx = np.maximum.accumulate(idx)
    return np.where(idx >= 0, ev[np.maximum(idx, 0)], 0)


def events(sid, st, en):
    """(forward events per row 0 .. M-1, backward events per index 1 .. M: the event at index k decides rows k - 1 and below)"""
    M = len(sid)
    sidx = np.concatenate(([0], sid, [0]))
    ch = sidx[1:] != sidx[:-1]                                 # ch[k] = SID[k] != SID[k - 1], k = 0 .. M
    fwd = np.where((st[:M] != 0) & ch[:M], 1, np.where((st[:M] == 0) & (en[:M] != 0) & ch[:M], 0, -1))
    bwd = np.where((en[1:] != 0) & ch[1:], 1, np.where((en[1:] == 0) & (st[1:] != 0) & ch[1:], 0, -1))
    return fwd, bwd


def reveal_mask(sid, st, en, no_fix=False, chunk_reset=0):
    """start_mask & end_mask per row.  no_fix: a forward walker that never takes an optimistic end_mask = 1 back (rows whose deciding event lies in a later
    64-row tile, or nowhere, keep 1).  chunk_reset: start_mask restarts from 0 at every chunk_reset-th row (a chunked launch without its repair)."""
    M = len(sid)
    fwd, bwd = events(sid, st, en)
    if chunk_reset:
        sm = np.concatenate([_fill(fwd[c:c + chunk_reset]) for c in range(0, M, chunk_reset)])
    else:
        sm = _fill(fwd)
    em = _fill(bwd, backward=True)
    if no_fix:
        k = np.where(bwd >= 0, np.arange(1, M + 1), 1 << 40)
        nxt = np.minimum.accumulate(k[::-1])[::-1]             # index of the deciding event of row j
        em = np.where(nxt // TILE > np.arange(M) // TILE, 1, em)
    return sm & em


def range_metric(sid, st, en, n):
    """(longest confirmed, longest taken back by an event, longest taken back by the string's end) optimistic range: the rows with start_mask = 1 between
    two consecutive backward events (or the last one and the string's end) that lie in an earlier 64-row tile than the resolving event"""
    M = len(sid)
    fwd, bwd = events(sid, st, en)
    sm = _fill(fwd)
    sm[n:] = 0
    cum = np.concatenate(([0], np.cumsum(sm)))
    ks = [int(k) + 1 for k in np.flatnonzero(bwd >= 0)]
    out = [0, 0, 0]
    lo = 0
    for k in ks:
        hi = min(k, (k // TILE) * TILE)                        # rows below the event's own tile
        if hi > lo:
            w = 0 if bwd[k - 1] == 1 else 1
            out[w] = max(out[w], int(cum[hi] - cum[lo]))
        lo = k
    hi = n if n >= M else (n // TILE) * TILE
    if hi > lo:
        out[2] = int(cum[hi] - cum[lo])
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# what the GPU tests launch (tests/test_carry_cpu.py checks every one of these batches on the CPU)
WITNESS_M = 2048                                               # the variant rows: eight forced chunks' worth of rows, 32 tiles
FORCED_CHUNK = 256                                             # kDbgForceSpec: chunks of 4 tiles
CHUNKED = [(2048, 256, "forced"), (8192, 256, "forced"),       # (M, rows per chunk, forced or the planner's own): 8 and 32 forced chunks,
           (8192, 1024, "8x16"), (65536, 2048, "32x32"), (131072, 4096, "32x64")]      # 8 x 16, 32 x 32 and 32 x 64 tiles
FORMS = {"one": dict(D=1), "second": dict(D=1, second=True), "two": dict(D=2), "three": dict(D=3), "big": dict(D=1, pad=200), "reduced": dict(D=1, reduced=True),
         "four_classes": dict(D=4, classes=20), "seven_wide": dict(D=7, classes=40), "eight": dict(D=8, classes=20),
         # the forms of the string-major rows of three and more defs (row_form of those rows at their fewest and most defs)
         "two_big": dict(D=2, pad=200), "three_big": dict(D=3, pad=200), "four_wide": dict(D=4, classes=40), "six_classes": dict(D=6, classes=20),
         "six_wide": dict(D=6, classes=40), "eight_wide": dict(D=8, classes=40), "nine": dict(D=9, classes=20), "twelve": dict(D=12, classes=20)}
SM_ROW_FORMS = ("two_big", "three_big", "four_wide", "six_classes", "six_wide", "eight_wide", "nine", "twelve")
BLOCK_BATCH = 65600                                            # rows that repeat their batch past one position-major block of 65536 strings: 320 rows (321 / 328)


def row_ms(shape):
    """the row counts of a variant row's lever batches: 2048 and a row count off the tile grid (tile_is_exact's second clause, a partial last tile), odd where
    the row takes any M — 2047 and 1001 for rows of M % 8 != 0 alone, 2040 and 1000 for rows of M % 16 == 8; the first alone where the variant needs 16384
    strings; 320 (321, 328) alone where it needs 65600 and more"""
    first = {"odd8": 2047, "m8x": 2040}.get(shape.m, WITNESS_M)
    if shape.min_batch >= BLOCK_BATCH:
        return ({"odd8": 321, "m8x": 328}.get(shape.m, 320),)
    if shape.min_batch:
        return (first,)
    return (first, {"any": 1001, "odd8": 1001, "m8x": 1000}.get(shape.m, 2000))


def row_form(shape, D):
    """scenario_batch's form for a row of the variant matrix (tests/test_variants_gpu.py ROWS) at D defs"""
    kw = dict(D=D)
    if shape.states == "big":
        kw["pad"] = 200
    elif shape.states == "pair":
        kw["reduced"] = True
    elif D == 1:
        kw["second"] = True
    if D >= 4:
        kw["classes"] = 40 if shape.s_max > 12 else 20      # (the class-table kernels take up to 32 byte classes per def; the multi-pass rows get the wide def)
    return kw


def repair_items(sid, st, en, n, chunk):
    """The chunks of one string that the chunked launch's stitch kernel queues for repair (csrc/hrx_kernel_spec.hip spec_stitch_kernel over what tile_masks leaves in a
    chunk's summary), modelled on the summed columns: chunk k is an item when start_mask = 1 comes into it (the walk assumed 0), or when it left rows pending with
    end_mask = 1 and the first deciding event behind it says 0.  Chunks that start at or behind the string's end are not looked at."""
    M = len(sid)
    fwd, bwd = events(sid, st, en)
    C = -(-M // chunk)
    pend, has_fwd, sm_out, dec = [0] * C, [0] * C, [0] * C, [0] * C
    for k in range(C):
        r0, r1 = k * chunk, min(M, (k + 1) * chunk)
        sm = _fill(fwd[r0:r1])
        has_fwd[k], sm_out[k] = int((fwd[r0:r1] >= 0).any()), int(sm[-1])
        q = [i for i in range(max(r0, 1), r1) if bwd[i - 1] >= 0]          # indices of the chunk's backward events (the event at i decides row i - 1)
        for t0 in range(r0, r1, TILE):                                    # the first tile that has an event or is exact says what decides the rows in front of the chunk
            exact = n <= t0 + TILE - 1 or t0 + TILE >= M
            inside = [i for i in q if t0 <= i < t0 + TILE]
            if inside or exact:
                dec[k] = (1 if bwd[inside[0] - 1] == 1 else 2) if inside else 2
                break
        lo = q[-1] if q else r0
        pend[k] = int(not exact and bool(sm[lo - r0:max(lo, min(n, r1)) - r0].any()))      # (exact: of the chunk's last tile)
    E, nxt = [0] * C, 0
    for k in range(C - 1, -1, -1):
        if k + 1 < C:
            E[k] = 1 if dec[k + 1] == 1 else 0 if dec[k + 1] == 2 else nxt
        nxt = E[k]
    items, sm = [], 0
    for k in range(C):
        if k * chunk >= n and k > 0:
            break
        if sm or (pend[k] and not E[k]):
            items.append(k)
        sm = sm_out[k] if has_fwd[k] else sm
    return items
