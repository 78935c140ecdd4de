"""The yardstick of LOOKUP COMPRESS (include/hrx.h hrx_lookup_compress_inputs_* / hrx_lookup_compress_table_*), in Python integers: the table rows from
OracleDefs.table_*_rows, the per-row states, ids and flags from the oracle's match_substrs (or from compact records, for rows that were tampered with), the
three tuples written out as src/lib.rs:218-283 writes them, and halo2's fold acc = acc * theta + e_i mod FR_MODULUS from 0.  Montgomery form is
x * 2^256 mod r.  Shares nothing with csrc/."""
import numpy as np

from fr_cases import FR_MODULUS

R = FR_MODULUS
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)
_MASK = (1 << 64) - 1


def limbs_of(x):
    """a 256-bit integer as 4 little-endian u64 limbs"""
    return [(x >> (64 * i)) & _MASK for i in range(4)]


def int_of(limbs):
    return sum(int(v) << (64 * i) for i, v in enumerate(limbs))


def theta_value(theta_int, canonical):
    """the challenge a call means by the 256-bit integer its limbs hold: taken mod r first; Montgomery limbs stand for x with x * 2^256 = limbs"""
    t = theta_int % R
    return t if canonical else t * MONT_INV % R


def cell_limbs(value, canonical):
    return limbs_of(value % R if canonical else value * MONT % R)


def fold(tup, theta):
    """halo2's commit_permuted: acc = acc * theta + e_i, from 0"""
    acc = 0
    for e in tup:
        acc = (acc * theta + int(e)) % R
    return acc


class CompressRef:
    def __init__(self, o):
        """o: an OracleDefs"""
        self.o, self.D = o, o.D
        self.tr = [[tuple(int(v) for v in row) for row in o.table_transition_rows(d)] for d in range(o.D)]
        self.ep = [[tuple(int(v) for v in row) for row in o.table_endpoint_rows(d)] for d in range(o.D)]
        self.dummy = [t[0][1] for t in self.tr]
        self._memo = {}

    def words(self):
        return (sum(len(t) + 2 * len(e) for t, e in zip(self.tr, self.ep)) + 3) // 4 * 4

    def layout(self):
        out, off = [], 0
        for t, e in zip(self.tr, self.ep):
            out.append({"trans": slice(off, off + len(t)), "start": slice(off + len(t), off + len(t) + len(e)),
                        "end": slice(off + len(t) + len(e), off + len(t) + 2 * len(e))})
            off += len(t) + 2 * len(e)
        return out

    def _cell(self, tup, theta, canonical):
        key = (tup, theta, canonical)
        if key not in self._memo:
            self._memo[key] = cell_limbs(fold(tup, theta), canonical)
        return self._memo[key]

    def tuples(self, n, M, character, state, sid, se, ee):
        """character [M]; state, sid, se, ee [D][M] integers -> [D][3][M] tuples: trans, start, end of every row as lib.rs:218-283 writes them"""
        out = []
        for d in range(self.D):
            dm = self.dummy[d]
            tr, st, en_ = [], [], []
            for r in range(M):
                en = 1 if r < n else 0
                cur, nxt = int(state[d][r]), int(state[d][r + 1]) if r + 1 < M else dm        # behind row M - 1: the cell nobody assigns, the dummy
                s, a, b, c = int(sid[d][r]), int(se[d][r]), int(ee[d][r]), int(character[r])
                tr.append((en * c, en * cur + (1 - en) * dm, en * nxt + (1 - en) * dm, en * s))
                st.append((a * s, a * cur + (1 - a) * dm, dm))
                en_.append((b * s, dm, b * nxt + (1 - b) * dm))
            out.append([tr, st, en_])
        return out

    def tuples_of_records(self, text, n, M, rec):
        """rec: (M, D) uint32 compact records of one string, as they lie (tampered or not)"""
        rec = np.asarray(rec, np.uint32).astype(np.int64)
        character = np.zeros(M, np.int64)
        character[:min(n, M)] = np.frombuffer(bytes(text[:min(n, M)]), np.uint8)
        return self.tuples(n, M, character, (rec & 0xffff).T, ((rec >> 16) & 0xff).T, ((rec >> 24) & 1).T, ((rec >> 25) & 1).T)

    def tuples_of_string(self, text, M):
        w = self.o.match_substrs(text, M)
        assert w["rc"] == 0
        return self.tuples(len(text), M, w["character"], w["state"], w["substr_id"], w["start_enable"], w["end_enable"])

    def cells_of_tuples(self, tuples, M, theta_int, canonical):
        """[3 D][M][4] uint64: the cells of one string"""
        theta = theta_value(theta_int, canonical)
        out = np.zeros((3 * self.D, M, 4), np.uint64)
        for d in range(self.D):
            for k in range(3):
                for r in range(M):
                    out[3 * d + k, r] = self._cell(tuples[d][k][r], theta, canonical)
        return out

    def cells_of_records(self, text, n, M, rec, theta_int, canonical):
        """[3 D][M][4] uint64; n > M: the string has no rows, zero cells"""
        if n > M:
            return np.zeros((3 * self.D, M, 4), np.uint64)
        return self.cells_of_tuples(self.tuples_of_records(text, n, M, rec), M, theta_int, canonical)

    def table_cells(self, theta_int, canonical):
        """[words()][4] uint64: per def trans[T_d], start[E_d], end[E_d] (both the fold of the endpoint row), the pad words zero cells"""
        theta = theta_value(theta_int, canonical)
        out = np.zeros((self.words(), 4), np.uint64)
        w = 0
        for t, e in zip(self.tr, self.ep):
            for row in t + e + e:
                out[w] = self._cell(row, theta, canonical)
                w += 1
        return out

    def hit(self, d, k, tup):
        """the word of a string's run that counts the tuple (the lowest table row equal to it), or None: it is in no row"""
        if not hasattr(self, "_at"):
            first = lambda rows: {row: i for i, row in reversed(list(enumerate(rows)))}
            self._at = [(first(t), first(e)) for t, e in zip(self.tr, self.ep)]
        lay = self.layout()[d]
        row = self._at[d][0 if k == 0 else 1].get(tuple(int(v) for v in tup))
        return None if row is None else (lay["trans"], lay["start"], lay["end"])[k].start + row
