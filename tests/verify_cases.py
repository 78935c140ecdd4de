"""The tamper catalogue of VERIFY (include/hrx.h hrx_verify_rows_*; csrc/hrx_verify.hpp): for a def set and M, base strings whose rows are clean, and one mutation
per string of one cell of those rows (or of the input) at the rows where verify_rows_kernel changes tile, stripe or rule — each with what it MUST do to the verdict
word, written from include/hrx.h and src/lib.rs:193-233, 387-519, 593-764 and from no checker's output.  Plain module (no GPU, no pytest), like tests/fr_cases.py and
tests/carry_defs.py: tests/test_verify_cases_cpu.py checks that the catalogue is what it claims, tests/test_verify_tamper_gpu.py runs it through every kernel form.

Def sets: carry_defs.lever_defs, so every def has six bytes of its own, no two defs ever flag one row, and the masked-row check is never silenced by `overlap`.
one / two / three / four / five / eight: one set per instantiation of the kernel (DT = 1, 2, 3, 4 and the runtime loop; D above 8 takes the loop of five).  big: one def
of 304 states (pad=300; the walk of 139 rows reaches state 92, the tables and their bitsets are those of 305 states).  second: one def with two substring ids, so the
bitset row `sid * ns` of an endpoint lookup is not row 0.

Base strings, one per length class n of LENS: every def owns one confirmed revealed range `s .. x e` of its own lever bytes — def 0 the rows 30 .. 34 (across
31 / 32), the last def but def 0 (def 0 itself in a one-def set) a range from 16 * ((n - 2) // 16) - 2 to min(n - 1, M - 3): across the last 16-row border below n
and, at M = 139, the last 8-row one; the other defs three rows each below row 30.  second: `t u u d`, a run of the second id, on rows 2 .. 5.  big: a run of the pad
byte from row 36 on, which walks the states 4, 5, 6 ...  The clean word of a base string is 0 in the one-def sets (every string ends on its `e`, in the accepted
state, or is full-length) and exactly the accept chain at row n in the others (def 0 is never in its accepted state where the string ends) — 0 where n == M.

Mutation kinds, each of which changes its cell (new = (old & keep) ^ flip):

    state      state ^ 1                    sid        tag ^ 1                     se   bit 24       fl2  bit 26         mask      cell ^ 0x0101
    state_out  state = 0xffff               sid_out    tag = 0xff                  ee   bit 25       fl7  bit 31         mask_sid  cell ^ 0x0100
    char       the input byte = carry_defs.UNDEF (no def has a transition for it)

and, in no string-major row: tail_rec / tail_msk (the rows M .. of the last quad / octet of a position-major buffer), gap (the rows M .. pitch - 1 of a pitched
string-major buffer), and the input bytes from n on: POISON_* in every such cell of every string at once, which must leave every word as it is.

What a mutation guarantees (`must_fail`: the bit is set, the word is not 0, its row field is as given — `eq`: exactly that row, `le`: at most that row, either after
the row of the clean word where that is lower):

    state*     r == 0                           FIRST_STATE   eq 0         the gate of row 0 (lib.rs:173-191); n >= 2, so row 0 is enabled
    state*     0 < r <= n                       TRANSITION    eq r - 1     the pair (r - 1, r): row r - 1 is enabled and its byte and state allow one next state
    state*     r > n                            PADDING       eq r         the dummy state behind row n (lib.rs:387-418)
    sid*       r < n, not (n == M, r == M - 1)  TRANSITION    le r         the table row of (byte, state) holds one tag
    sid*       r >= n                           PADDING       le r         no tag from row n on
    se, ee     r < n                            FLAGS         le r         the flags are functions of (tag, state, next state), none of which moved
    se, ee     r >= n                           PADDING       le r         no flag from row n on
    fl2, fl7   any                              PADDING       le r         flag bits that do not exist
    mask*      any                              MASK          le r         a cell that is neither 0 nor what the range reveals
    char       r < n, not (n == M, r == M - 1)  TRANSITION    eq r         no table row for the byte

`must_not_matter` (the word equals the clean string's): char at r >= n (enable * char is 0), char at (n == M, r == M - 1) — that row's lookup reads the cell
Rotation::next of the last row, which match_substrs never assigns, and is left out; no base string reveals row M - 1 — and every tail / gap cell.
`open`: sid* at (n == M, r == M - 1), for the same reason; the table guarantees nothing there and the torch checker decides."""
import numpy as np

import carry_defs as cd

M_ROWS = 139                      # 35 quads (odd: the stripes hold 18 and 17), 18 octets; M % 32 = M % 16 = 11, M % 8 = M % 4 = 3
LENS = (64, 101, 139)             # on a border of every tile size, mid-tile, n == M
SETS = {"one": dict(D=1), "two": dict(D=2), "three": dict(D=3), "four": dict(D=4), "five": dict(D=5), "eight": dict(D=8), "big": dict(D=1, pad=300),
        "second": dict(D=1, second=True)}
FIRST_STATE, TRANSITION, FLAGS, PADDING, MASK = 1, 4, 64, 128, 256          # HRX_VERIFY_* of include/hrx.h
ALL_ONES = 0xffffffff
# kind -> (buffer, keep, flip): new = (old & keep) ^ flip
OPS = {"state": ("rec", ALL_ONES, 1), "state_out": ("rec", 0xffff0000, 0xffff), "sid": ("rec", ALL_ONES, 1 << 16), "sid_out": ("rec", 0xff00ffff, 0xff << 16),
       "se": ("rec", ALL_ONES, 1 << 24), "ee": ("rec", ALL_ONES, 1 << 25), "fl2": ("rec", ALL_ONES, 1 << 26), "fl7": ("rec", ALL_ONES, 1 << 31),
       "mask": ("msk", 0xffff, 0x0101), "mask_sid": ("msk", 0xffff, 0x0100), "char": ("chr", 0, cd.UNDEF)}
RECORD_KINDS = tuple(k for k, v in OPS.items() if v[0] == "rec")
ROW_KINDS = tuple(k for k, v in OPS.items() if v[0] != "rec")
POISON_KINDS = ("tail_rec", "tail_msk", "gap")
POISON_REC, POISON_MSK, POISON_CHAR = 0xffffffff, 0xffff, cd.UNDEF      # a state, tag and flags out of every table; a cell no range reveals; a byte no def knows


def defs_text(name):
    return cd.lever_defs(**SETS[name])


def edge_rows(n, M):
    return sorted(r for r in {0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, n - 2, n - 1, n, n + 1, M - 2, M - 1} if 0 <= r < M)


def base_string(name, n, M=M_ROWS):
    """(bytes of the string, [(def, first row, last row) of every confirmed range])"""
    kw = SETS[name]
    D = kw["D"]
    assert M >= 48 and 40 <= n <= M
    s = cd._Str(n)
    ranges = []

    def confirmed(a, b, k):
        assert a + 2 <= b <= min(n - 1, M - 2) and all(a > hi + 1 or b < lo - 1 for _, lo, hi in ranges)
        s.put(a, "s", k)
        s.put(b - 1, "xe", k)
        ranges.append((k, a, b))
    near = D - 1
    small = [k for k in range(1, D) if k != near]
    for i, k in enumerate(small):
        confirmed(2 + 4 * i, 4 + 4 * i, k)
    confirmed(30, 34, 0)
    confirmed(16 * ((n - 2) // 16) - 2, min(n - 1, M - 3), near)
    if kw.get("second"):
        for i, c in enumerate((cd.SECOND[0], cd.SECOND[1], cd.SECOND[1], cd.SECOND[2])):
            s.raw(2 + i, c)
        ranges.append((0, 2, 5))
    if kw.get("pad"):
        for r in range(36, ranges[1][1] - 1):          # (one filler byte behind the run brings the walk back to state 0, where `s` is a start)
            s.raw(r, cd.PADB)
    return s.v, ranges


def expectation(kind, r, n, M):
    """(class, guaranteed bit, ("eq" | "le", row) or None): the table of the module's docstring"""
    last_unassigned = n == M and r == M - 1
    if kind in ("state", "state_out"):
        return ("must_fail", FIRST_STATE, ("eq", 0)) if r == 0 else ("must_fail", TRANSITION, ("eq", r - 1)) if r <= n else ("must_fail", PADDING, ("eq", r))
    if kind in ("sid", "sid_out"):
        if last_unassigned:
            return "open", 0, None
        return ("must_fail", TRANSITION, ("le", r)) if r < n else ("must_fail", PADDING, ("le", r))
    if kind in ("se", "ee"):
        return ("must_fail", FLAGS, ("le", r)) if r < n else ("must_fail", PADDING, ("le", r))
    if kind in ("fl2", "fl7"):
        return "must_fail", PADDING, ("le", r)
    if kind in ("mask", "mask_sid"):
        return "must_fail", MASK, ("le", r)
    assert kind == "char"
    return ("must_fail", TRANSITION, ("eq", r)) if r < n and not last_unassigned else ("must_not_matter", 0, None)


class Catalogue:
    """chars (B, stride) u8 and lens (B,) u32 of the clean strings; muts[i] = (string, kind, row, def, (keep, flip)), one per string, with cls[i], bit[i], row[i] of
    expectation(); fillers: the strings no mutation touches (two in front of and two behind every length class); base[b]: the filler that holds string b's clean rows;
    poison: the (kind, class) of the never-judged cells, which hold for every string"""

    def __init__(self, name, M=M_ROWS):
        self.name, self.M, self.defs_t, self.D = name, M, defs_text(name), SETS[name]["D"]
        rows, lens, self.muts, self.cls, self.bit, self.row, self.fillers, base, self.ranges = [], [], [], [], [], [], [], [], {}
        for n in LENS:
            v, self.ranges[n] = base_string(name, n, M)
            first = len(rows)

            def add():
                rows.append(v); lens.append(n); base.append(first)
                return len(rows) - 1
            self.fillers += [add(), add()]
            for r in edge_rows(n, M):
                for kind in RECORD_KINDS + ROW_KINDS:
                    for d in (range(self.D) if kind in RECORD_KINDS else (0,)):
                        self.muts.append((add(), kind, r, d, OPS[kind][1:]))
                        c, bit, row = expectation(kind, r, n, M)
                        self.cls.append(c); self.bit.append(bit); self.row.append(row)
            self.fillers += [add(), add()]
        self.B, self.stride = len(rows), (M + 1 + 15) // 16 * 16
        self.chars = np.zeros((self.B, self.stride), np.uint8)
        for b, v in enumerate(rows):
            self.chars[b, :len(v)] = v
        self.lens, self.base = np.array(lens, np.uint32), np.array(base)
        self.poison = [(k, "must_not_matter") for k in POISON_KINDS]

    def cells(self, buffer):
        """the mutations of one buffer ("rec", "msk", "chr") as arrays: (string, row, def, keep, flip)"""
        sel = [m for m in self.muts if OPS[m[1]][0] == buffer]
        col = lambda f: np.array([f(m) for m in sel], np.int64)
        return col(lambda m: m[0]), col(lambda m: m[2]), col(lambda m: m[3]), col(lambda m: m[4][0]), col(lambda m: m[4][1])

    def apply(self, rec, msk, chars):
        """the whole list on string-major rows (B, M, D) u32, (B, M) u16 and the input (B, stride) u8: changed copies"""
        rec, msk, chars = rec.copy(), msk.copy(), chars.copy()
        b, r, d, keep, flip = self.cells("rec")
        rec[b, r, d] = (rec[b, r, d] & keep.astype(np.uint32)) ^ flip.astype(np.uint32)
        b, r, d, keep, flip = self.cells("msk")
        msk[b, r] = (msk[b, r] & keep.astype(np.uint16)) ^ flip.astype(np.uint16)
        b, r, d, keep, flip = self.cells("chr")
        chars[b, r] = (chars[b, r] & keep.astype(np.uint8)) ^ flip.astype(np.uint8)
        return rec, msk, chars

    def counts(self):
        return {c: self.cls.count(c) for c in ("must_fail", "must_not_matter", "open")}


def base_batch(name, copies=24, M=M_ROWS):
    """(chars, lens): the clean base strings alone, the length classes in turn"""
    v = [base_string(name, n, M)[0] for n in LENS]
    B = copies * len(LENS)
    chars = np.zeros((B, (M + 1 + 15) // 16 * 16), np.uint8)
    lens = np.zeros(B, np.uint32)
    for b in range(B):
        chars[b, :len(v[b % 3])] = v[b % 3]
        lens[b] = len(v[b % 3])
    return chars, lens


def small_batch(D, M, B=70, seed=0):
    """(chars, lens) for a short circuit: B strings of random lever bytes of D defs (every byte has a transition in every state of every def), n cycling over
    0, 1, M - 1, M; the stride is one 16-byte chunk more than M needs"""
    rng = np.random.default_rng(1000 * D + M + seed)
    pool = np.frombuffer(b"".join(cd.LEVERS[:D]), np.uint8)
    chars = np.zeros((B, (M + 15) // 16 * 16 + 16), np.uint8)
    lens = np.array([(0, 1, M - 1, M)[b % 4] for b in range(B)], np.uint32)
    lens = np.minimum(lens, M)
    for b in range(B):
        chars[b, :lens[b]] = pool[rng.integers(0, len(pool), size=int(lens[b]))]
    return chars, lens
