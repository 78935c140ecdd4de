"""The yardstick of LOOKUP PRODUCT (include/hrx.h hrx_lookup_invert_table_* / hrx_lookup_product_*), in Python integers mod FR_MODULUS with pow(x, -1, r) as
the inversion: the rule of the header transcribed literally, over cells whose limbs are turned into integers by compress_ref's conventions and index columns
that a caller takes from hra.permuted_lookup_columns (numpy) or hands in as they are.  Shares nothing with csrc/."""
import numpy as np

from compress_ref import R, MONT, MONT_INV, cell_limbs, int_of, theta_value


def value_of(limbs, canonical):
    """the element a reduced cell stands for"""
    x = int_of(limbs)
    assert x < R
    return x if canonical else x * MONT_INV % R


def values_of(cells, canonical):
    return [value_of(c, canonical) for c in np.asarray(cells).reshape(-1, 4)]


def challenge_value(limbs, canonical):
    """a shift, beta or gamma: any 256-bit value, taken mod r first"""
    return theta_value(int_of(limbs), canonical)


def inverse_table(run_cells, bins, shift_limbs, canonical):
    """[W][4] uint64: inv[w] = (S[w] + c)^-1, the zero cell where S[w] + c == 0 and in the pad words [bins, W)"""
    c = challenge_value(shift_limbs, canonical)
    out = np.zeros((len(run_cells), 4), np.uint64)
    for w in range(bins):
        s = (value_of(run_cells[w], canonical) + c) % R
        out[w] = cell_limbs(pow(s, -1, R) if s else 0, canonical)
    return out


def product_column(A_in, n, M, k, off, T, S, inv_b, inv_g, a_idx, s_idx, n_rows, beta, gamma):
    """One lookup (k = 0 trans, 1 start, 2 end) of one string of n characters, everything integers: A_in the M input values, S / inv_b / inv_g the values of
    the run's table and of its two inverse tables, a_idx / s_idx the index columns.  Returns Z[0 .. n_rows]."""
    Z = [1]
    for i in range(n_rows):
        if i >= M or n > M or (n == M and i == M - 1 and k in (0, 2)):
            A = S[off]
        else:
            A = A_in[i]
        Si = S[off + i] if i < T else S[off]
        ia, is_ = int(a_idx[i]), int(s_idx[i])
        if not (off <= ia < off + T) or not (off <= is_ < off + T):
            term = 0
        else:
            term = (A + beta) * (Si + gamma) % R * inv_b[ia] % R * inv_g[is_] % R
        Z.append(Z[-1] * term % R)
    return Z


def product(lookups, lens, M, in_cells, a_idx, s_idx, n_rows, table, beta, gamma, canonical, b_begin=0, strings=None):
    """lookups: [(column, slice into a run)] in hrx_lookup_num_columns' order; in_cells uint64 [3 D][b_count][M][4]; a_idx, s_idx [3 D][b_count][>= n_rows];
    table uint64 (W, 4) or (b_count, W, 4); beta, gamma uint64 (4,) or (b_count, 4).  The inverse tables are the yardstick's own (inverse_table).  Returns
    (z uint64 [3 D][b_count][n_rows + 1][4], open uint32 [b_count], Z integers {(column, string): list}); strings: the strings of the window to compute."""
    ncols, b_count = in_cells.shape[0], in_cells.shape[1]
    bins = max(sl.stop for _, sl in lookups)
    z = np.zeros((ncols, b_count, n_rows + 1, 4), np.uint64)
    opened = np.zeros(b_count, np.uint32)
    ints, memo = {}, {}
    for b in (range(b_count) if strings is None else strings):
        run = table[b] if table.ndim == 3 else table
        bl, gl = (beta[b], gamma[b]) if beta.ndim == 2 else (beta, gamma)
        key = (b if table.ndim == 3 else 0, b if beta.ndim == 2 else 0)
        if key not in memo:
            memo[key] = (values_of(run, canonical), values_of(inverse_table(run, bins, bl, canonical), canonical),
                         values_of(inverse_table(run, bins, gl, canonical), canonical))
        S, inv_b, inv_g = memo[key]
        bv, gv = challenge_value(bl, canonical), challenge_value(gl, canonical)
        for col, sl in lookups:
            Z = product_column(values_of(in_cells[col, b], canonical), int(lens[b_begin + b]), M, col % 3, sl.start, sl.stop - sl.start, S, inv_b, inv_g,
                               a_idx[col, b], s_idx[col, b], n_rows, bv, gv)
            ints[(col, b)] = Z
            z[col, b] = [cell_limbs(v, canonical) for v in Z]
            if Z[n_rows] != 1:
                opened[b] |= np.uint32(1 << col)
    return z, opened, ints
