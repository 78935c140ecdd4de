"""The yardstick of LOOKUP COUNTS (include/hrx.h hrx_lookup_counts_*), in numpy and a dict: the table rows from OracleDefs.table_*_rows, the per-row states, ids
and flags from the oracle's match_substrs (or from compact records, for rows that were tampered with), the three tuples formed as src/lib.rs:218-283 writes
them, and a lookup of the whole tuple with the lowest table row first.  Shares nothing with csrc/hrx_lookup.hpp."""
import numpy as np


def _first_row_of(rows):
    out = {}
    for k, row in enumerate(rows):
        out.setdefault(tuple(int(v) for v in row), k)
    return out


class LookupRef:
    def __init__(self, o):
        """o: an OracleDefs"""
        self.o, self.D = o, o.D
        self.tr = [o.table_transition_rows(d) for d in range(o.D)]
        self.ep = [o.table_endpoint_rows(d) for d in range(o.D)]
        self.tr_at = [_first_row_of(t) for t in self.tr]
        self.ep_at = [_first_row_of(e) for e in self.ep]
        self.dummy = [int(t[0][1]) for t in self.tr]

    def words(self):
        return (sum(len(t) + 2 * len(e) for t, e in zip(self.tr, self.ep)) + 3) // 4 * 4

    def layout(self):
        out, off = [], 0
        for t, e in zip(self.tr, self.ep):
            out.append({"trans": slice(off, off + len(t)), "start": slice(off + len(t), off + len(t) + len(e)),
                        "end": slice(off + len(t) + len(e), off + len(t) + 2 * len(e))})
            off += len(t) + 2 * len(e)
        return out

    def count_cells(self, n, M, character, state, sid, se, ee):
        """character [M]; state, sid, se, ee [D][M] integers -> (run of words() counts, misses per def and lookup [D][3])"""
        run = np.zeros(self.words(), np.uint32)
        miss = np.zeros((self.D, 3), np.int64)
        lay = self.layout()
        for d in range(self.D):
            dm = self.dummy[d]
            for r in range(M):
                en = 1 if r < n else 0
                unassigned = r == M - 1 and n == M           # Rotation::next of row M - 1 is a cell match_substrs never assigns
                cur, nxt = int(state[d][r]), int(state[d][r + 1]) if r + 1 < M else dm
                s, a, b, c = int(sid[d][r]), int(se[d][r]), int(ee[d][r]), int(character[r])
                looks = [("start", self.ep_at[d], (a * s, a * cur + (1 - a) * dm, dm), 1)]
                if not unassigned:
                    looks.append(("trans", self.tr_at[d], (en * c, en * cur + (1 - en) * dm, en * nxt + (1 - en) * dm, en * s), 0))
                    looks.append(("end", self.ep_at[d], (b * s, dm, b * nxt + (1 - b) * dm), 2))
                for name, at, tup, k in looks:
                    row = at.get(tup)
                    if row is None:
                        miss[d, k] += 1
                    else:
                        run[lay[d][name].start + row] += 1
        return run, miss

    def count_string(self, text, M):
        """a string the defs accept transitions for: the cells are the oracle's match_substrs"""
        w = self.o.match_substrs(text, M)
        assert w["rc"] == 0
        return self.count_cells(len(text), M, w["character"], w["state"], w["substr_id"], w["start_enable"], w["end_enable"])

    def count_records(self, text, n, M, rec):
        """rec: (M, D) uint32 compact records of one string, as they lie (tampered or not)"""
        rec = np.asarray(rec, np.uint32).astype(np.int64)
        character = np.zeros(M, np.int64)
        character[:min(n, M)] = np.frombuffer(bytes(text[:min(n, M)]), np.uint8)
        return self.count_cells(n, M, character, (rec & 0xffff).T, ((rec >> 16) & 0xff).T, ((rec >> 24) & 1).T, ((rec >> 25) & 1).T)
