"""Cases and the reference for the field-cell tests (hrx_fr_columns_device*, fr_columns_kernel of csrc/hrx_kernel.hip).  Plain module (no GPU, no pytest):
tests/test_fr_cases_cpu.py asserts what it claims from the oracle alone, tests/test_fr_cells_gpu.py runs the kernel against it.

The reference is built from the ORACLE's compact rows (OracleDefs.witness_batch): expected_columns unpacks them into the [4 + 4 D][B][M] integer columns of
include/hrx.h, cells_of sends every value through a 65536-entry table of F::from(v) made with Python integers.  Nothing here calls the library under test.

sweep_def(L) is a definition whose walk reaches any state 0..L within two bytes, so that a batch of 40 short strings holds every state value up to the 2046 of
the largest one-def config: the values >= 256 are the ones fr_columns_kernel computes in place instead of reading from its LDS table."""
import numpy as np

FR_MODULUS = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001     # BN254 scalar field
SWEEP_L = 2045            # the largest L a one-def config takes: its table has L + 3 = 2048 rows
SWEEP_L2 = 1020           # two such defs: 2 * 1023 = 2046 rows
POISON = 0xA5
GUARD = 4096              # bytes before and behind the cells


# ---- definitions -------------------------------------------------------------------------------------------------------------------------------
def sweep_def(L, lo=0, hi=6):
    """(allstr_text, [substr_text]): states 0..L, first state 0, accepted state L; byte 97 s -> (s + 1) % (L + 1), byte 98 s -> s, byte 128 + k
    any state -> 64 k (k < 32, 64 k <= L).  One substring definition: the increment pairs (s, s + 1) with lo <= s % 10 < hi, starting at the s % 10 == lo
    sources and ending at the s % 10 == hi targets."""
    lines = ["0", str(L), str(L)]
    for s in range(L + 1):
        lines.append("%d %d 97" % (s, (s + 1) % (L + 1)))
        lines.append("%d %d 98" % (s, s))
        for k in range(32):
            if 64 * k <= L:
                lines.append("%d %d %d" % (s, 64 * k, 128 + k))
    pairs = [(s, s + 1) for s in range(L) if lo <= s % 10 < hi]
    starts = sorted({s for s, _ in pairs if s % 10 == lo})
    ends = sorted({t for _, t in pairs if t % 10 == hi % 10})
    sub = "\n".join(["%d" % (hi - lo + 2), "0", "%d" % (L + 1), " ".join(map(str, starts)) + " ", " ".join(map(str, ends)) + " "] + ["%d %d" % p for p in pairs]) + "\n"
    return "\n".join(lines) + "\n", [sub]


def sweep_defs(D):
    """the definition texts of the one-def sweep (L = 2045) or the two-def sweep (L = 1020 twice, substring picks that never share a row)"""
    if D == 1:
        return [sweep_def(SWEEP_L)]
    assert D == 2
    return [sweep_def(SWEEP_L2, 0, 6), sweep_def(SWEEP_L2, 6, 9)]


def sweep_batch(L, B=40, M=72, stride=80, seed=11):
    """(chars (B, stride) uint8, lens (B,) uint32): 32 strings `jump, then 'a' to the end` whose lengths alternate between M and M - 8 .. M - 1 (string b jumps to
    64 (b % jumps); with fewer than 32 jump bytes the later strings walk a few 'a' first), and 8 random mixes of {97, 97, 97, 98, jumps} of lengths 0..M, one empty."""
    assert B == 40 and stride % 16 == 0 and stride > M
    rng = np.random.default_rng(seed)
    jumps = min(32, L // 64 + 1)
    chars = np.zeros((B, stride), np.uint8)
    lens = np.zeros(B, np.uint32)
    for b in range(32):
        lead = b // jumps * 3
        s = b"a" * lead + bytes([128 + b % jumps]) + b"a" * (stride - 1 - lead)
        chars[b] = np.frombuffer(s, np.uint8)
        lens[b] = M if b % 2 == 0 else M - 8 + (b // 2) % 8
    pool = np.array([97, 97, 97, 98] + [128 + k for k in range(jumps)], np.uint8)
    for b in range(32, B):
        n = 0 if b == 35 else int(rng.integers(1, M + 1))
        chars[b, :n] = pool[rng.integers(0, len(pool), size=n)]
        lens[b] = n
    lens[39] = M
    chars[39, :M] = pool[rng.integers(0, len(pool), size=M)]
    return chars, lens


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------
def expected_columns(orec, omsk, chars, lens, M, D):
    """[4 + 4 D][B][M] int64: the integer content of every column (include/hrx.h: 0 char_enable, 1 characters, 2+4d states[d], 3+4d substr_ids[d],
    4+4d start_enable[d], 5+4d end_enable[d], 2+4D masked_characters, 3+4D all_substr_ids) out of the oracle's witness_batch rows
    (records u32: state | id << 16 | start << 24 | end << 25; masked u16: character | id << 8)."""
    B = len(lens)
    assert orec.shape == (B, M, D) and omsk.shape == (B, M)
    cols = np.zeros((4 + 4 * D, B, M), np.int64)
    live = np.arange(M)[None, :] < np.minimum(np.asarray(lens, np.int64), M)[:, None]
    w = min(M, chars.shape[1])
    cols[0] = live
    cols[1, :, :w] = np.where(live[:, :w], chars[:, :w], 0)
    rec = orec.astype(np.int64)
    for d in range(D):
        cols[2 + 4 * d] = rec[:, :, d] & 0xffff
        cols[3 + 4 * d] = (rec[:, :, d] >> 16) & 0xff
        cols[4 + 4 * d] = (rec[:, :, d] >> 24) & 1
        cols[5 + 4 * d] = (rec[:, :, d] >> 25) & 1
    msk = omsk.astype(np.int64)
    cols[2 + 4 * D] = msk & 0xff
    cols[3 + 4 * D] = msk >> 8
    return cols


def columns_of_match_substrs(o, chars, lens, M, strings):
    """[4 + 4 D][len(strings)][M] int64 from OracleDefs.match_substrs (the oracle's restatement of lib.rs:311-773), string by string; every rc must be 0"""
    D = o.D
    out = np.zeros((4 + 4 * D, len(strings), M), np.int64)
    for i, b in enumerate(strings):
        c = o.match_substrs(bytes(chars[b, :lens[b]]), M)
        assert c["rc"] == 0, (b, c["rc"])
        seq = [c["enable"], c["character"]]
        for d in range(D):
            seq += [c["state"][d], c["substr_id"][d], c["start_enable"][d], c["end_enable"][d]]
        seq += [c["masked_char"], c["masked_substr_id"]]
        for k, col in enumerate(seq):
            out[k, i] = np.asarray(col, np.int64)
    return out


_LUT = {}


def lut(canonical):
    """(65536, 4) uint64: the limbs of F::from(v), Montgomery form (v << 256) % r in Python integers, or canonical [v, 0, 0, 0]"""
    if canonical not in _LUT:
        t = np.zeros((65536, 4), np.uint64)
        if canonical:
            t[:, 0] = np.arange(65536)
        else:
            mask = (1 << 64) - 1
            for v in range(65536):
                x = (v << 256) % FR_MODULUS
                t[v] = (x & mask, (x >> 64) & mask, (x >> 128) & mask, x >> 192)
        t.setflags(write=False)
        _LUT[canonical] = t
    return _LUT[canonical]


def cells_of(columns, canonical, table=None):
    """columns [...] of integers 0..65535 -> [..., 4] uint64 limbs"""
    columns = np.asarray(columns)
    assert columns.min(initial=0) >= 0 and columns.max(initial=0) < 65536
    return (lut(canonical) if table is None else table)[columns]


def first_difference(got, want):
    """None, or where `got` [n_cols][b][M][4] first differs from `want`"""
    got, want = np.asarray(got).view(np.uint64), np.asarray(want).view(np.uint64)
    if got.shape != want.shape:
        return "shape %s, want %s" % (got.shape, want.shape)
    if np.array_equal(got, want):
        return None
    c, b, r, k = (int(x) for x in np.argwhere(got != want)[0])
    return "column %d string %d row %d limb %d: got %#x want %#x (%d cells differ)" % (c, b, r, k, int(got[c, b, r, k]), int(want[c, b, r, k]),
                                                                                       int((got != want).any(axis=-1).sum()))


# ---- guarded device cells ----------------------------------------------------------------------------------------------------------------------
def guarded_cells(torch, dev, n_cols, b_count, M, offset=0):
    """(cells, raw): a poisoned byte buffer with GUARD bytes before and behind the [n_cols][b_count][M][4] int64 cells, the cells 16-byte aligned
    (offset: bytes to shift them by, for the misaligned case).  guards_intact(raw, cells) checks both guards."""
    nbytes = n_cols * b_count * M * 32
    raw = torch.full((GUARD + nbytes + GUARD + 16,), POISON, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0 and GUARD % 16 == 0
    cells = raw[GUARD + offset:GUARD + offset + nbytes].view(torch.int64).view(n_cols, b_count, M, 4)
    return cells, raw


def guards_intact(raw, cells, what=""):
    nbytes = cells.numel() * 8
    lo = cells.data_ptr() - raw.data_ptr()
    for name, part in (("before", raw[:lo]), ("behind", raw[lo + nbytes:])):
        bad = (part != POISON).nonzero()
        assert bad.numel() == 0, "%s: a write %s the cells, guard byte %d" % (what, name, int(bad[0]))


def untouched(raw):
    return bool((raw == POISON).all())


# ---- host-side layouts (include/hrx.h), index by index ------------------------------------------------------------------------------------------
PM_BLOCK = 65536


def to_position_major(rec, msk):
    """(B, M, D) records and (B, M) masked rows -> the flat HRX_LAYOUT_POSITION_MAJOR host buffers: per block of 65536 strings records
    [ceil(M/4)][D][nb][4], masked [ceil(M/8)][nb][8], blocks back to back; rows >= M of the last quad / octet zero"""
    B, M, D = rec.shape
    q4, q8 = (M + 3) // 4, (M + 7) // 8
    r4 = np.zeros((B, q4 * 4, D), rec.dtype)
    r4[:, :M] = rec
    m8 = np.zeros((B, q8 * 8), msk.dtype)
    m8[:, :M] = msk
    recs, msks = [], []
    for k0 in range(0, B, PM_BLOCK):
        nb = min(PM_BLOCK, B - k0)
        recs.append(np.ascontiguousarray(r4[k0:k0 + nb].reshape(nb, q4, 4, D).transpose(1, 3, 0, 2)).reshape(-1))
        msks.append(np.ascontiguousarray(m8[k0:k0 + nb].reshape(nb, q8, 8).transpose(1, 0, 2)).reshape(-1))
    return np.concatenate(recs), np.concatenate(msks)


def chars_position_major(chars):
    """(B, stride) -> the flat HRX_LAYOUT_INPUT_POSITION_MAJOR host buffer ([stride/16][nb][16] per block)"""
    B, stride = chars.shape
    parts = []
    for k0 in range(0, B, PM_BLOCK):
        c = chars[k0:k0 + PM_BLOCK]
        parts.append(np.ascontiguousarray(c.reshape(c.shape[0], stride // 16, 16).transpose(1, 0, 2)).reshape(-1))
    return np.concatenate(parts)


# ---- the other cases ----------------------------------------------------------------------------------------------------------------------------
CFG_1 = [["regex1_test_lookup.txt", ["substr1_test_lookup.txt"]]]
CFG_A = CFG_1 + [["regex2_test_lookup.txt", ["substr2_test_lookup.txt"]]]
EDGE_MS = (1, 3, 4, 5, 8, 31, 32, 33, 127, 128, 129, 511, 512, 513, 1025)
_LOWER = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", np.uint8)
_PLANT1, _PLANT2 = b"email was meant for @y.", b" Also for x."


def edge_batch(M):
    """regex1 + regex2, five strings of lengths {0, 1, M - 1, M, M // 2}: lowercase noise with `email was meant for @y.` and ` Also for x.` planted where
    they fit; stride > M, a multiple of 16"""
    rng = np.random.default_rng(1000 + M)
    stride = (M + 16) // 16 * 16
    lens = np.array([0, 1, M - 1, M, M // 2], np.uint32)
    chars = np.zeros((5, stride), np.uint8)
    for b, n in enumerate(int(x) for x in lens):
        chars[b, :n] = _LOWER[rng.integers(0, len(_LOWER), size=n)]
        text = _PLANT1 + _PLANT2 if n >= 35 else _PLANT2 if n >= 12 else b""
        at = int(rng.integers(0, n - len(text) + 1)) if b % 2 else n - len(text)      # (even strings: the match ends at the string's last row)
        chars[b, at:at + len(text)] = np.frombuffer(text, np.uint8)
    return chars, lens, stride


def header_lines(B, stride, seed, from_lines=True):
    """B strings of 40 .. stride - 3 noise bytes with one or two short header lines planted — `to:`, `subject:Send ...` and, with from_lines, `from:` in the header
    definition's and in regex3's form — short enough for the 72-row cases (a whole block of synth.headers_planted takes more than 63 bytes)"""
    from halo2_regex_amd import synth
    rng = np.random.default_rng(seed)
    chars, lens = np.zeros((B, stride), np.uint8), np.zeros(B, np.uint32)
    w = lambda lo, hi: bytes(_LOWER[rng.integers(0, 26, size=int(rng.integers(lo, hi + 1)))])
    addr = lambda: w(1, 3) + b"@" + w(1, 3) + b"." + w(2, 2)
    for b in range(B):
        n = int(rng.integers(40, stride - 2))
        chars[b, :n] = synth.ALPHABET98[rng.integers(0, len(synth.ALPHABET98), size=n)]
        lines = [b"\r\nfrom:" + w(1, 4) + b" <" + addr() + b">\r\n", b"\r\nto:" + addr() + b"\r\n",
                 b"\r\nsubject:Send " + str(int(rng.integers(1, 1000))).encode() + b" " + w(2, 3).upper() + b" to " + addr() + b"\r\n",
                 b"\r\nfrom:" + w(1, 4) + b"<" + w(1, 4) + b"@" + w(1, 4) + b".com>\r\n"]
        if not from_lines:
            lines = [lines[1], lines[2], lines[1], lines[2]]
        text = lines[b % 4] + (lines[(b + 1) % 4] if b % 3 else b"")
        if len(text) > n:
            text = lines[b % 4]
        at = int(rng.integers(0, n - len(text) + 1))
        chars[b, at:at + len(text)] = np.frombuffer(text, np.uint8)
        lens[b] = n
    return chars, lens


def defcount_batch(names, B=70, M=72):
    """70 strings for the configs of 4 .. 13 defs, planted as tests/test_parity_gpu.py plants them: 50 reveal-stress strings (regex1 / regex2 / regex3 pieces)
    and 20 with header lines.  Two kinds of config cannot take the reveal-stress strings (the oracle reports them): one that holds the partial example DFA
    beside regex1 takes only prefixes of the literal `email was meant for @` (one more byte and both flag the row: status 2); one that holds regex1 / regex2 twice
    flags every such match twice.  Their 50 strings are those prefixes, and header lines, instead."""
    from halo2_regex_amd import synth
    assert B == 70
    files = [a for a, _ in names]
    chars, lens = synth.reveal_stress(50, M - 8, seed=37)
    stride = chars.shape[1]
    if "ex_allstr.txt" in files:
        lit = np.frombuffer(b"email was meant for @", np.uint8)
        chars[:], lens[:] = 0, 0
        for b in range(50):
            lens[b] = b % (len(lit) + 1)
            chars[b, :lens[b]] = lit[:lens[b]]
    from_lines = not {"regex3_test_lookup.txt", "header_from_lookup.txt"} <= set(files)      # (both flag a `from:` line: status 2)
    if "ex_allstr.txt" not in files and len(set(files)) < len(files):
        chars, lens = header_lines(50, stride, 7, from_lines)
    h_c, h_l = header_lines(20, stride, 5, from_lines)
    chars, lens = np.concatenate([chars, h_c]), np.concatenate([lens, h_l]).astype(np.uint32)
    wide = np.zeros((B, (M + 16) // 16 * 16), np.uint8)
    wide[:, :stride] = chars
    return wide, lens


BIG_B, BIG_M, BIG_STRIDE = PM_BLOCK + 300, 8, 16
BIG_RANGES = ((65400, 300), (65535, 2), (BIG_B - 1, 1), (30000, 35800), (BIG_B, 0))      # (b_begin, b_count); the fourth crosses the launch cut at 30000 + 32768 and the block border
BIG_SHORT = BIG_RANGES[:3]
BIG_SWEEP_L, BIG_SWEEP_BYTES = 40, (97, 97, 97, 98, 128)      # sweep_def(40) on the big batch's shape: revealed rows on both sides of string 65536 (regex1 reveals nothing within 8 rows)


def big_batch(alphabet=None):
    """65536 + 300 strings of at most 8 bytes: lengths 0..8 in turn, prefixes of `email wa`, lowercase noise and `@x.` at every offset — the same mix on both
    sides of string 65536, every string different from its neighbours.  alphabet: bytes to draw from instead (the small sweep definition)."""
    rng = np.random.default_rng(65536)
    B, M = BIG_B, BIG_M
    lens = (np.arange(B) % 9).astype(np.uint32)
    if alphabet is not None:
        pool = np.frombuffer(bytes(alphabet), np.uint8)
        chars = np.zeros((B, BIG_STRIDE), np.uint8)
        chars[:, :M] = pool[rng.integers(0, len(pool), size=(B, M))]
        return chars, lens
    chars = np.zeros((B, BIG_STRIDE), np.uint8)
    chars[:, :M] = _LOWER[rng.integers(0, 26, size=(B, M))]
    pre = np.frombuffer(b"email wa", np.uint8)
    k = (np.arange(B) // 9) % 4
    chars[k == 1, :M] = pre                                  # the literal's first eight bytes: states 1 .. 8
    for off in range(6):
        rows = np.nonzero((k == 2) & ((np.arange(B) // 36) % 6 == off))[0]
        chars[rows[:, None], off + np.arange(3)[None, :]] = np.frombuffer(b"@x.", np.uint8)
    return chars, lens


# At M = 8 every row has r >> 3 == 0 and r >> 4 == 0, so in the masked-row index ((r >> 3) * nb + bl) and in the position-major chars index ((r >> 4) * nb + bl)
# the block's string count nb is multiplied by zero: only the records index (quad 1) meets nb = 300.  Nineteen rows reach octets 1 and 2 and chars group 1, with a
# partial last quad and octet.  (With sweep_def a revealed part needs one more byte behind it, so row M - 1 is never revealed: 19 rows, not 17, let row 16, the
# first of octet 2, be revealed.)
TALL_M, TALL_STRIDE = 19, 32
TALL_PLANTED = (PM_BLOCK - 1, PM_BLOCK, PM_BLOCK + 1, BIG_B - 2, BIG_B - 1)


def tall_batch():
    """65536 + 300 strings of at most 19 bytes for sweep_def(40): lengths 0..19 in turn, random mixes of BIG_SWEEP_BYTES; the strings beside the block border and
    the batch's last two are full-length `k filler bytes, jump to 0, then a`, each with another k (k = 10 reveals rows 11 .. 16, the first row of octet 2
    included) and such that rows 16 .. 18 of one never equal what a neighbouring slot of the chars buffer holds"""
    rng = np.random.default_rng(17)
    B, M = BIG_B, TALL_M
    pool = np.frombuffer(bytes(BIG_SWEEP_BYTES), np.uint8)
    lens = (np.arange(B) % (M + 1)).astype(np.uint32)
    chars = np.zeros((B, TALL_STRIDE), np.uint8)
    chars[:, :M] = pool[rng.integers(0, len(pool), size=(B, M))]
    for b, text in zip(TALL_PLANTED, (b"\x80" + b"a" * 18, b"b" * 10 + b"\x80" + b"a" * 8, b"b" * 9 + b"\x80" + b"a" * 9, b"bbb\x80" + b"a" * 12 + b"bbb", b"ab" * 5 + b"\x80" + b"a" * 8)):
        chars[b, :M] = np.frombuffer(text, np.uint8)
        lens[b] = M
    return chars, lens


def gather_with_nb(flat, group, per_string, B, b, r, nb_of):
    """The element of row r of string b in a position-major buffer of `group`-row slots ([per_string slots][nb][group] per block of 65536 strings), read as
    fr_columns_kernel indexes it but with nb_of(nb) in place of the block's string count: what a kernel with a wrong nb would read"""
    blk0 = b // PM_BLOCK * PM_BLOCK
    nb = min(PM_BLOCK, B - blk0)
    return flat[(blk0 * per_string + (r // group) * nb_of(nb) + (b - blk0)) * group + r % group]


def big_sample():
    """at least 200 strings of the big batch: both sides of string 65536 and of every range edge, then a fixed random draw"""
    rng = np.random.default_rng(3)
    edges = {0, BIG_B - 1, PM_BLOCK - 1, PM_BLOCK, 30000 + 32768 - 1, 30000 + 32768}
    for b0, n in BIG_RANGES:
        edges |= {b0 - 1, b0, b0 + n - 1, b0 + n}
    edges = {b for b in edges if 0 <= b < BIG_B}
    return sorted(edges | set(int(x) for x in rng.integers(0, BIG_B, size=220)))


BAD_STRINGS = (3, 9, 40)      # the out-of-contract batch: strings 3 and 40 have lens = M + 1, string 9 a byte without a transition


def bad_batch(M=72):
    """the 70 strings of defcount_batch(CFG_A) with three out-of-contract strings planted (BAD_STRINGS)"""
    chars, lens = defcount_batch(CFG_A, 70, M)
    chars, lens = chars.copy(), lens.copy()
    for b in (3, 40):
        chars[b, :M + 1] = _LOWER[np.arange(M + 1) % 26]
        lens[b] = M + 1
    lens[9] = max(int(lens[9]), 20)
    chars[9, :20] = _LOWER[np.arange(20) % 26]
    chars[9, 11] = 250
    return chars, lens
