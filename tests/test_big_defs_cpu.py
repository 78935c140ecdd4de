"""TWO BIG TABLES IN ONE RUN, on the host (tests/big_defs.py): the properties the device matrix of test_big_defs_gpu.py depends on, asserted from the
context's own reports, and the host twins of counts, permute, invert and product held to their independent yardsticks — lookup_ref.py, the numpy
construction, Python integers — on these def sets, so that the yardsticks of the device tests are validated where no device is.  No device."""
import numpy as np
import pytest

import big_defs as bd
import halo2_regex_amd as hra
import product_ref as pr
from compress_ref import R, cell_limbs
from test_lookup_cpu import check_against_ref
from test_permute_cpu import check_against_numpy, t_max
from test_product_cpu import Chain

NONE = hra.HRX_DEVICE_NONE
LOOKUP_BITS = hra.VERIFY_TRANSITION | hra.VERIFY_START_LOOKUP | hra.VERIFY_END_LOOKUP


@pytest.mark.parametrize("name", bd.SETS)
def test_the_matrix_is_not_empty(name):
    """four passes or more; a def that begins strictly inside a later pass; a def whose bins touch three passes; an endpoint lookup across a pass border; two
    lookups beyond a chunk whose fill lists — for the counts the device tests use — are longer than a chunk and differ from each other and between strings; a
    workspace of B W 4 bytes; and what the tamper rounds rely on"""
    M = bd.M_SMALL
    cfg = bd.configure(name, M, NONE)
    chars, lens = bd.batch(M)
    B = len(lens)
    p = bd.properties(cfg, B)
    lay = cfg.lookup_layout()
    assert p["G"] == 1 and p["passes"] >= 4 and p["pass_words"] * p["passes"] >= p["W"] > p["pass_words"] * (p["passes"] - 1)
    assert cfg.lookup_group(1 << 20) == (1, p["passes"])                               # the planner never groups strings where it cuts passes
    assert p["begins_mid_pass"] and p["begins_mid_pass"][-1] == cfg.num_defs - 1
    if name == "big-big":           # every property in one set: def 0's trans, start and end bins begin in three passes, its end lookup lies across a border
        assert p["touches_three"] == [0] and p["ranges_apart"] == [0] and (0, "end") in p["straddling_endpoint"]
    if name == "small-big-big":
        assert p["touches_three"] == [1]
    assert len(p["big"]) == 2 and all(col % 3 == 0 for col, sl in p["big"]) and p["T"] == 65537 and p["T"] > 21 * p["plan"]["chunk_rows"]
    assert len(p["multi_chunk"]) == cfg.num_defs            # (the small def's transition table is beyond a chunk too)
    assert p["plan"]["groups"] == 1 and p["workspace"] == B * p["W"] * 4
    if name == "big-big":
        assert bd.properties(bd.configure(name, 64, NONE), B)["pass_words"] == p["pass_words"]      # M does not enter
    # the small def lies across a border when it stands between the big ones
    small = {"big-small-big": 1, "small-big-big": 0}.get(name)
    if name == "big-small-big":
        assert bd.pass_of(lay[small]["trans"].start, p["pass_words"]) != bd.pass_of(lay[small]["end"].stop - 1, p["pass_words"])
    # batch: the lengths, three strings and more with status 0 in every def
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    ok = [b for b in range(B) if int(st[b]) & 0xff == 0]
    assert {0, 1, 7, M - 1, M, M + 1} == set(int(n) for n in lens) and 6 <= B <= 8 and len(ok) >= 3 and set(ok) == set(range(B)) - {bd.LONG}
    # the fill lists of the honest counts: longer than a chunk, different in the two lookups and from string to string
    counts, misses = cfg.lookup_counts_host(chars, lens, rec)
    fills = {(col, b): bd.fill_list(counts[b][sl]) for col, sl in p["big"] for b in ok}
    chunk = p["plan"]["chunk_rows"]
    assert all(len(f) > chunk for f in fills.values())
    (c0, _), (c1, _) = p["big"]
    assert all(not np.array_equal(fills[c0, b], fills[c1, b]) for b in ok if lens[b] > 1)        # (one byte from state 0: the same row of both)
    assert not np.array_equal(fills[c0, ok[-1]], fills[c0, ok[-2]]) and not np.array_equal(fills[c1, ok[-1]], fills[c1, ok[-2]])
    names, hand, over = bd.hand_made(cfg, p["T"])
    hf = [[bd.fill_list(hand[i][sl]) for col, sl in p["big"]] for i in range(3)]
    assert all(not np.array_equal(a, b) for a, b in hf) and not np.array_equal(hf[0][0], hf[1][0])
    assert len(hf[0][0]) > chunk and len(hf[0][1]) > chunk and len(hf[1][0]) > chunk and len(hf[2][1]) > chunk    # ("all rows but row 0" fills with row 0 alone)
    # the tamper rounds: every kind in def 0 and in the def that begins mid-pass, at rows 0, M // 2 and M - 2
    mid = p["begins_mid_pass"][-1]
    seen = {c for rnd in bd.tamper_rounds(M, mid) for b, c in rnd.items() if b != 2}
    assert seen == {(k, r, d) for k in bd.BITS for r in (0, M // 2, M - 2) for d in (0, mid)} and mid != 0


@pytest.mark.parametrize("M", bd.M_COUNTS)
@pytest.mark.parametrize("name", bd.SETS)
def test_counts_host_twin_against_the_reference(oracle, name, M):
    """honest rows, then every tamper round: counts and misses against lookup_ref.py on every string, the sums a prover relies on per def, misses nonzero
    exactly where verify_rows_host reports a lookup bit; a string without rows has all-zero bins and misses 0xffffffff whatever its records hold"""
    cfg = bd.configure(name, M, NONE)
    ref = bd.lookup_ref(oracle, name)
    chars, lens = bd.batch(M)
    B = len(lens)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    have = [b for b in range(B) if b != bd.LONG]
    mid = bd.properties(cfg, B)["begins_mid_pass"][-1]
    lay = cfg.lookup_layout()
    kinds = np.zeros((cfg.num_defs, 3), np.int64)
    for rnd in [{}] + bd.tamper_rounds(M, mid):
        r2 = rec.copy()
        for b, (kind, row, d) in rnd.items():
            r2[b, row, d] ^= np.uint32(bd.BITS[kind])
        counts, misses = cfg.lookup_counts_host(chars, lens, r2)
        check_against_ref(cfg, ref, chars, lens, r2, st if not rnd else np.ones(B, np.uint64), counts, misses, sample=have)
        assert not counts[bd.LONG].any() and misses[bd.LONG] == bd.TOO_LONG
        for fill in (0, 0xffffffff):
            r3 = r2.copy()
            r3[bd.LONG] = fill
            c3, m3 = cfg.lookup_counts_host(chars, lens, r3)
            assert np.array_equal(c3, counts) and np.array_equal(m3, misses)
        verdict = cfg.verify_rows_host(chars, lens, r2, msk)
        assert np.array_equal(misses[have] != 0, (verdict[have] & np.uint64(LOOKUP_BITS)) != 0)
        if not rnd:
            assert not misses[have].any()
        for b in rnd:
            run, miss = ref.count_records(chars[b], int(lens[b]), M, r2[b])
            kinds += miss
    assert kinds[0].all() and kinds[mid].all(), "the rounds make the transition, the start and the end lookup of def 0 and of the def that begins mid-pass miss"


def test_permute_host_twin_against_the_numpy_construction():
    cfg = bd.configure("big-big", bd.M_SMALL, NONE)
    T = t_max(cfg)
    for n_rows in (T, 65 * 1024 + 1):
        names, counts, over = bd.hand_made(cfg, n_rows)
        res = cfg.lookup_permute_host(counts, n_rows, out=("idx",))
        assert np.array_equal(check_against_numpy(cfg, counts, n_rows, res), over) and np.array_equal(res["overflow"], over), names


@pytest.mark.parametrize("name", ["big-big", "big-small-big"])
def test_chain_host_twin_against_python_integers(oracle, name):
    """the host chain on the strings of the device chain test: honest ones, string 4 with a state of the last def changed, string 6 with an end flag of def 0
    set, string 5 without rows.  The closing property; `open` has exactly the bits of the lookups that missed; the inverse tables at samples and at every def
    border; ONE string — a tampered one, of big + big — through product_ref in Python integers"""
    M = bd.M_SMALL
    cfg = bd.configure(name, M, NONE)
    ref = bd.lookup_ref(oracle, name)
    D = cfg.num_defs
    chars, lens = bd.batch(M)
    rec, msk, st = cfg.witness_batch_host(chars, np.minimum(lens, M))
    rec[4, M // 2, D - 1] ^= np.uint32(bd.BITS["state"])
    rec[6, 0, 0] ^= np.uint32(bd.BITS["ee"])
    n_rows = t_max(cfg) + 1
    ch = Chain(cfg, chars, lens, rec, n_rows, seed=6)
    res = ch.product()
    for b in (4, 6):
        miss = ref.count_records(chars[b], int(lens[b]), M, rec[b])[1]
        bits = sum(1 << (3 * d + k) for d in range(D) for k in range(3) if miss[d, k])
        assert bits and res["open"][b] == bits, (b, miss)
    assert res["open"][4] >> 3 * (D - 1) & 1 and res["open"][6] & 4
    honest = ch.honest()
    assert honest == [0, 1, 2, 3, bd.LONG, 7] and not res["open"][honest].any()
    one = np.array(cell_limbs(1, False), np.uint64)
    assert (res["z"][:, honest, n_rows] == one).all()
    assert ch.misses[bd.LONG] == bd.TOO_LONG and not ch.counts[bd.LONG].any() and not ch.inputs[:, bd.LONG].any()
    check_inverse_samples(cfg, ch.table, ch.beta, ch.inv_beta)
    check_inverse_samples(cfg, ch.table, ch.gamma, ch.inv_gamma)
    if name == "big-big":
        z, opened, ints = ch.ref(strings=[4])
        assert np.array_equal(res["z"][:, 4, :n_rows + 1], z[:, 4]) and opened[4] == res["open"][4]


def check_inverse_samples(cfg, table, shift, inv, canonical=False):
    """40 sampled words of each big run and the words on both sides of every def border against pow(x, -1, r)"""
    lay = cfg.lookup_layout()
    rng = np.random.default_rng(5)
    words = set()
    for l in lay:
        sl = l["trans"]
        if sl.stop - sl.start > 60000:
            words |= set(int(w) for w in rng.integers(sl.start, sl.stop, 40))
        words |= {l["trans"].start, l["end"].stop - 1}
    c = pr.challenge_value(shift, canonical)
    for w in sorted(words):
        s = (pr.value_of(table[w], canonical) + c) % R
        assert pr.value_of(inv[w], canonical) == (pow(s, -1, R) if s else 0), w
    assert not inv[lay[-1]["end"].stop:].any()
