"""Edge operands of the field arithmetic under FR NTT (csrc/hrx_fr.h fr_add, fr_sub, fr_mul, fr_pow_u32 as csrc/hrx_ntt.hpp uses them), as Python integers and
sharing nothing with csrc/.  A transform of size 2 is the field's add and sub — its table is the single entry one — and with a shift one fr_mul more, so any
operand pair goes through the arithmetic as a column of a k = 1 call.  Everything here is in STORED-value space: a cell holds the 256-bit integer v below r,
whatever it stands for; fr_mul(x, y) = x y R^-1 mod r on stored values, a Montgomery shift s is the stored g = s mod r, a canonical one g = (s mod r) R.
  forward  (a, b) -> (a + b g / R, a - b g / R)
  inverse  (a, b) -> ((a + b) / 2, (a - b) / 2 * g / R)
and without a shift g / R is 1."""
import itertools

import numpy as np

import ntt_ref as nr
from compress_ref import R, MONT, MONT_INV

POISON64 = 0x5A5A5A5A5A5A5A5A
INV2 = (R + 1) // 2
ALL_ONES = int("30644e71" + "ffffffff" * 7, 16)                 # the largest all-ones pattern below r
E = [
    0, 1, 2, 3, R - 1, R - 2, R - 3, (R - 1) // 2, (R + 1) // 2,
    MONT, R - MONT, MONT * MONT % R,
    2**32 - 1, 2**32, 2**64 - 1, 2**64, 2**128 - 1, 2**128, 2**192, 2**224 - 1, 2**253, 2**253 + 1,
    R - 2**32, R - 2**64, R - 2**128, R - 2**192, R >> 64 << 64,                       # ... and r with its low limb cleared
    ALL_ONES,
    int("ffffffff00000000" * 4, 16) % R, int("00000000ffffffff" * 4, 16) % R,          # alternating limbs (the first is above r as it stands)
    0xf0000001, R - 0xf0000001,                                                        # r's own low limb: the Montgomery quotient m is 0xffffffff
    2**252 - 1,
]
assert len(E) == len(set(E)) == 33 and all(0 <= v < R for v in E)
UNREDUCED = [R, R + 1, 2**256 - 1]                               # shifts only: taken mod r first, and g = 0 gives g^0 = 1, g^1 = 0
SIX = [0, 1, R - 1, (R + 1) // 2, MONT, ALL_ONES]                # the operands of the k = 2 tuples


def limbs_array(values):
    """uint64 [len][4]: the little-endian limbs of 256-bit integers"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint64).reshape(-1, 4).copy()


def tuple_cells(tuples):
    """uint64 [len][pitch][4]: a column per tuple; pitch 4 or more, the entries behind the tuple poisoned"""
    width = len(tuples[0])
    cells = np.full((len(tuples), max(width, 4), 4), POISON64, np.uint64)
    cells[:, :width] = limbs_array([v for t in tuples for v in t]).reshape(len(tuples), width, 4)
    return cells


def pairs(values=E):
    return list(itertools.product(values, repeat=2))


def shift_limbs(s):
    """the limbs a call is handed for the 256-bit integer s, as they are: not reduced, not converted"""
    return None if s is None else limbs_array([s])[0]


def size_2(a, b, s, inverse, canonical):
    """the two stored outputs of the k = 1 transform of the stored pair (a, b) with the shift limbs s (None: none)"""
    g = 1 if s is None else s % R * (MONT if canonical else 1) * MONT_INV % R
    if not inverse:
        return (a + b * g) % R, (a - b * g) % R
    return (a + b) * INV2 % R, (a - b) * INV2 * g % R


def first_wrong_pair(got, prs, s, inverse, canonical):
    """None where the cells got[len(prs)][>= 2][4] are size_2 of every pair, else what the first wrong one is"""
    want = limbs_array([v for a, b in prs for v in size_2(a, b, s, inverse, canonical)]).reshape(len(prs), 2, 4)
    if np.array_equal(got[:, :2], want):
        return None
    c, o = (int(v) for v in np.argwhere((got[:, :2] != want).any(axis=2))[0])
    return "pair %d (a = %#x, b = %#x), output %d, shift %s, %s, %s: got %#x, want %#x" % (
        c, prs[c][0], prs[c][1], o, "none" if s is None else hex(s), "inverse" if inverse else "forward", "canonical" if canonical else "Montgomery",
        sum(int(v) << (64 * i) for i, v in enumerate(got[c, o])), sum(int(v) << (64 * i) for i, v in enumerate(want[c, o])))


def naive_of_tuples(tuples, k, inverse, canonical, g):
    """uint64 [len][2^k][4]: ntt_ref.naive of every tuple of stored values, read in the limb form, with the shift g (an element; None: none)"""
    want = [nr.naive(nr.values_of(limbs_array(t), canonical), k, inverse, 1 if g is None else g) for t in tuples]
    return nr.cells_of([v for w in want for v in w], canonical).reshape(len(tuples), 1 << k, 4)


def tile_columns(k, seed):
    """uint64 [3][2^k][4], stored values from E in a seeded order: a column of them; one whose second half is the negation of its first, x[i + n/2] = r - x[i]
    — every stage-0 sum is exactly r (or 0 + 0) and must give the zero cell; one whose halves are equal — every stage-0 difference is 0"""
    n = 1 << k
    rng = np.random.default_rng(seed)
    pick = lambda count: [E[i] for i in rng.integers(0, len(E), count)]
    whole, half_a, half_b = pick(n), pick(n // 2), pick(n // 2)
    return np.stack([limbs_array(whole), limbs_array(half_a + [(R - v) % R for v in half_a]), limbs_array(half_b + half_b)])
