"""The yardstick of LOOKUP QUOTIENT in Python integers (include/hrx.h LOOKUP QUOTIENT; the five steps of csrc/hrx_quotient.hpp's header as they are written
there, sharing nothing with csrc/ — no regrouping, no powers of y): the fold over the extended coset, the vanishing inverse, and the selectors by direct
evaluation of the Lagrange bases at the coset points."""
import functools

from compress_ref import R
from ntt_ref import omega


def points(ext_k, g):
    """the extended coset: point j is g w_ext^j"""
    w = omega(ext_k)
    out, p = [], g % R
    for _ in range(1 << ext_k):
        out.append(p)
        p = p * w % R
    return out


def t_inv(k, ext_k, g):
    """1 / (g^n w_ext^(n c) - 1) for c < 2^(ext_k - k); 0 where the denominator is 0"""
    n, w = 1 << k, omega(ext_k)
    out = []
    for c in range(1 << (ext_k - k)):
        d = (pow(g, n, R) * pow(w, n * c, R) - 1) % R
        out.append(pow(d, -1, R) if d else 0)
    return out


@functools.lru_cache(maxsize=None)
def selectors(k, ext_k, n_rows, g):
    """(l0, l_last, l_active) on the coset of g: L_i(x) = w^i (x^n - 1) / (n (x - w^i)), the basis polynomial of row i, evaluated at every point; l_last is row
    n_rows, l_active the sum over rows [0, n_rows).  g outside the subgroup (no point is a row's w^i)."""
    n, w = 1 << k, omega(k)
    n_inv = pow(n, -1, R)
    rows = [pow(w, i, R) for i in range(n)]

    def basis(i, x, xn1):
        return rows[i] * xn1 % R * n_inv % R * pow((x - rows[i]) % R, -1, R) % R

    l0, l_last, l_active = [], [], []
    for x in points(ext_k, g):
        xn1 = (pow(x, n, R) - 1) % R
        l0.append(basis(0, x, xn1))
        l_last.append(basis(n_rows, x, xn1))
        l_active.append(sum(basis(i, x, xn1) for i in range(n_rows)) % R)
    return l0, l_last, l_active


def fold(k, ext_k, lookups, sel, beta, gamma, y, h_in=None, t=None):
    """one string.  lookups: a list of dicts of integer lists A, Ap, Sp, Z, S over the N points; sel = (l0, l_last, l_active); h_in a list or None (zero);
    t: t_inv's list to divide, or None.  The five steps, in halo2's order, for every lookup in turn."""
    N, rot = 1 << ext_k, 1 << (ext_k - k)
    l0, l_last, l_active = sel
    out = []
    for j in range(N):
        v = h_in[j] if h_in is not None else 0
        jn, jp = (j + rot) % N, (j - rot) % N
        for c in lookups:
            A, Ap, Sp, Z, S = c["A"], c["Ap"], c["Sp"], c["Z"], c["S"]
            v = (v * y + (1 - Z[j]) * l0[j]) % R
            v = (v * y + (Z[j] * Z[j] - Z[j]) * l_last[j]) % R
            v = (v * y + (Z[jn] * (Ap[j] + beta) * (Sp[j] + gamma) - Z[j] * (A[j] + beta) * (S[j] + gamma)) * l_active[j]) % R
            v = (v * y + (Ap[j] - Sp[j]) * l0[j]) % R
            v = (v * y + (Ap[j] - Sp[j]) * (Ap[j] - Ap[jp]) * l_active[j]) % R
        out.append(v * t[j % rot] % R if t is not None else v)
    return out
