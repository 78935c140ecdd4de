"""The yardstick of FR NTT in Python integers (include/hrx.h FR NTT; the rule of csrc/hrx_ntt.hpp transcribed from its two formulas, sharing nothing with
csrc/): a naive O(n^2) transform straight from the sums, an independent iterative transform for the sizes the naive one is too slow for (decimation in
FREQUENCY over a list, where the library decimates in time), Horner evaluation for spot checks, and the constants recomputed from the field."""
import numpy as np

from compress_ref import R, MONT, MONT_INV, cell_limbs, int_of

S = 28
GENERATOR = 7
ROOT_OF_UNITY = pow(GENERATOR, (R - 1) >> S, R)
ZETA = pow(GENERATOR, (R - 1) // 3, R)          # a primitive cube root of one: the PSE fork's coset generators are its powers
assert (R - 1) % (1 << S) == 0 and ((R - 1) >> S) % 2 == 1
assert pow(ROOT_OF_UNITY, 1 << (S - 1), R) == R - 1 and pow(ROOT_OF_UNITY, 1 << S, R) == 1      # of order exactly 2^28


def omega(k):
    return pow(ROOT_OF_UNITY, 1 << (S - k), R)


def values_of(cells, canonical):
    """the integers of an array of cells [..][4]"""
    flat = np.asarray(cells, np.uint64).reshape(-1, 4)
    out = [int_of(c) for c in flat]
    return out if canonical else [x * MONT_INV % R for x in out]


def cells_of(values, canonical):
    return np.array([cell_limbs(v, canonical) for v in values], np.uint64).reshape(-1, 4)


def naive(x, k, inverse=False, g=1):
    """the two sums as they are written: x a list of n_in <= 2^k integers, the entries behind it zero"""
    n, w = 1 << k, omega(k)
    if not inverse:
        xs = [pow(g, i, R) * v % R for i, v in enumerate(x)]
        return [sum(v * pow(w, i * j % n, R) for i, v in enumerate(xs)) % R for j in range(n)]
    wi, ninv = pow(w, -1, R), pow(n, -1, R)
    return [pow(g, i, R) * ninv * sum(v * pow(wi, i * j % n, R) for j, v in enumerate(x)) % R for i in range(n)]


def iterative(x, k, inverse=False, g=1):
    """the same by decimation in frequency (natural order in, bit-reversed out, then un-reversed)"""
    n = 1 << k
    w = omega(k) if not inverse else pow(omega(k), -1, R)
    a = [0] * n
    p = 1
    for i, v in enumerate(x):
        a[i] = v * p % R if not inverse else v
        if not inverse:
            p = p * g % R
    half = n >> 1
    wl = w
    while half >= 1:
        tw = [1] * half
        for j in range(1, half):
            tw[j] = tw[j - 1] * wl % R
        for base in range(0, n, 2 * half):
            for j in range(half):
                u, v = a[base + j], a[base + j + half]
                a[base + j] = (u + v) % R
                a[base + j + half] = (u - v) * tw[j] % R
        wl = wl * wl % R
        half >>= 1
    out = [0] * n
    for i in range(n):
        out[int(format(i, "0%db" % k)[::-1], 2)] = a[i]
    if inverse:
        ninv, p = pow(n, -1, R), 1
        for i in range(n):
            out[i] = out[i] * ninv % R * p % R
            p = p * g % R
    return out


def eval_at(coeffs, point):
    """the polynomial with these coefficients (lowest first) at `point`, by Horner"""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * point + c) % R
    return acc


__all__ = ["R", "MONT", "S", "ROOT_OF_UNITY", "ZETA", "omega", "values_of", "cells_of", "naive", "iterative", "eval_at"]
