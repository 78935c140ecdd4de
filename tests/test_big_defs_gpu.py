"""TWO BIG TABLES IN ONE RUN and STRINGS WITHOUT ROWS, on the device (the cases of tests/big_defs.py, whose properties test_big_defs_cpu.py asserts): what one
synthetic 256-state DFA on honest rows never showed the lookup chain.

  counts in passes     four passes, a def that begins mid-pass, a def over three passes, an endpoint lookup across a border: sm, pm-in, planes and a window,
                       M = 19 and 64, against the host twin word for word and lookup_ref.py on every string; then one mutation per string on the device copy —
                       non-zero misses out of the transition, start and end lookups of a def whose ranges lie in different passes, against the reference's
                       sum, the device verdict's lookup bits and the sums a prover relies on
  strings without rows lens = M + 1 and 0xffffffff at the first and last place of a group, alone in the last group, first of a window, both sides of the
                       position-major block border; every row form; G > 1 and G = 1; the records of that string filled with 0xffffffff and with 0: the run
                       is all zero, misses 0xffffffff, and no output word depends on the fill
  permute              two multi-chunk fill lists per string side by side in the workspace: device counts (honest, tampered) and hand-made ones, different
                       patterns in the two big lookups of one string, an overflow in the second big def beside sound lookups; n_rows = T, T + 1, 65 x 1024 and
                       + 1; indices only, one table run, a run per string; a workspace one byte short
  the chain            counts, compress, permute, two inverts, product on the device over two (and three) defs' runs: against the host twin limb for limb,
                       `open` of a tampered string against the lookups the reference says missed, the inverse tables against pow(x, -1, r) at samples and at
                       every def border, one string through Python integers

Every device output lies between two poisoned 4-KiB guards.  No test provokes a fault: a string without rows is one the header defines, and every value put
into a record is one the host twin and verify_rows_kernel's tamper matrix have seen."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import big_defs as bd
import fr_cases as fc
import halo2_regex_amd as hra
import product_ref as pr
from compress_ref import cell_limbs
from test_big_defs_cpu import check_inverse_samples
from test_compress_gpu import on_device
from test_lookup_cpu import check_against_ref
from test_lookup_gpu import against_ref, batch as ragged_batch, device_counts, guarded as lk_guarded, intact as lk_intact, largest_group_from, same_as_host, LOOKUP_BITS
from test_permute_cpu import lookups_of, t_max
from test_permute_gpu import Out, host_table, same_as_host as permute_same_as_host
from test_product_cpu import challenges
from test_product_gpu import Z, device_invert
from test_verify_gpu import Rows, defs_of_files, defs_of_text, CFG_A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NO_ROW = 0xffffffff
FORMS = ("sm", "sm-pitched", "pm", "pm-in", "planes")


def set_lens(rows, lens):
    rows.lens = np.ascontiguousarray(lens, np.uint32)
    rows.d_lens = torch.from_numpy(rows.lens.view(np.int32).copy()).to(DEV)


def rows_of(cfg, form, chars, lens):
    """the device rows of a batch; a string with lens > M is witnessed at M characters (honest rows lie in its cells) and gets its length afterwards"""
    rows = Rows(cfg, form, chars, np.minimum(lens, cfg.max_chars_size))
    set_lens(rows, lens)
    return rows


def fill_records(rows, strings, value):
    """every record cell of `strings` on the device, all defs, set to `value`"""
    b, r, d = (a.reshape(-1) for a in np.meshgrid(np.asarray(strings), np.arange(rows.M), np.arange(rows.D), indexing="ij"))
    which, idx = rows.rec_cells(b, r, d)
    rows.update(rows.rec_buffers(), which, idx, np.zeros(len(b), np.int64), np.full(len(b), value, np.int64))


# ---- counts in passes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", bd.M_COUNTS)
@pytest.mark.parametrize("name", bd.SETS)
def test_counts_in_four_passes(oracle, name, M):
    cfg = bd.configure(name, M, 0)
    ref = bd.lookup_ref(oracle, name)
    chars, lens = bd.batch(M)
    B = len(lens)
    assert cfg.lookup_group(B)[0] == 1 and cfg.lookup_group(B)[1] >= 4
    have = [b for b in range(B) if b != bd.LONG]
    for form in ("sm", "pm-in", "planes"):
        rows = rows_of(cfg, form, chars, lens)
        got, gm = same_as_host(rows)
        against_ref(rows, ref, got, gm, have)
        assert not gm[have].any() and not got[bd.LONG].any() and gm[bd.LONG] == bd.TOO_LONG
        assert np.array_equal(rows.host_rows()[0][have], cfg.witness_batch_host(chars, np.minimum(lens, M))[0][have])
        w, wm = same_as_host(rows, 2, 5)                           # a window that begins behind the batch's first string
        against_ref(rows, ref, w, wm, [2, 3, 4, 6], b_begin=2)
        assert np.array_equal(w, got[2:7]) and np.array_equal(wm, gm[2:7])


@pytest.mark.parametrize("form", ["sm", "pm-in", "planes"])
@pytest.mark.parametrize("name,M", [(n, bd.M_SMALL) for n in bd.SETS] + [("big-big", 64)])
def test_tampered_rows_miss_in_every_pass(oracle, name, M, form):
    """the rounds of big_defs.tamper_rounds on the device copy.  A def's misses are counted once, in the pass that holds its first bin: def 0 of big + big has
    its transition, start and end bins in three passes, the last def begins mid-pass"""
    cfg = bd.configure(name, M, 0)
    ref = bd.lookup_ref(oracle, name)
    chars, lens = bd.batch(M)
    B = len(lens)
    have = [b for b in range(B) if b != bd.LONG]
    mid = bd.properties(cfg, B)["begins_mid_pass"][-1]
    kinds = np.zeros((cfg.num_defs, 3), np.int64)
    for rnd in bd.tamper_rounds(M, mid):
        rows = rows_of(cfg, form, chars, lens)
        for b, (kind, row, d) in rnd.items():
            rows.xor_rec(b, row, d, bd.BITS[kind])
        got, gm = same_as_host(rows)
        w, wm = same_as_host(rows, 2, 5)                           # the window form of the call, on tampered rows
        assert np.array_equal(w, got[2:7]) and np.array_equal(wm, gm[2:7])
        rec, msk = rows.host_rows()
        check_against_ref(cfg, ref, chars, lens, rec, np.ones(B, np.uint64), got, gm, sample=have)      # equal runs, equal sums of misses, the sums per def
        verdict = rows.verify()
        assert np.array_equal(gm[have] != 0, (verdict[have] & np.uint64(LOOKUP_BITS)) != 0), (rnd, gm, verdict)
        assert gm[bd.LONG] == bd.TOO_LONG and not got[bd.LONG].any()
        for b in rnd:
            miss = ref.count_records(chars[b], int(lens[b]), M, rec[b])[1]
            kinds += miss
            assert int(gm[b]) == miss.sum()
    assert kinds[0].all() and kinds[mid].all(), "misses out of the transition, the start and the end lookup of def 0 and of the def that begins mid-pass"


# ---- strings without rows -----------------------------------------------------------------------------------------------------------------------
def no_rows(rows, longs, windows):
    """longs: {string: lens value}.  The windows' counts and misses with the records of those strings filled with 0xffffffff and with 0: equal to the host twin
    (every neighbour too), the same words under both fills, and as the header says for the strings themselves"""
    lens = rows.lens.copy()
    for b, v in longs.items():
        lens[b] = v
    set_lens(rows, lens)
    assert (rows.d_lens.cpu().numpy().view(np.uint32) == lens).all() and all(v > rows.M for v in longs.values())
    res = []
    for fill in (0xffffffff, 0):
        fill_records(rows, sorted(longs), fill)
        res.append([same_as_host(rows, b0, n) for b0, n in windows])
        seen = 0
        for (b0, n), (got, gm) in zip(windows, res[-1]):
            n = rows.B - b0 if n is None else n
            for b in longs:
                if b0 <= b < b0 + n:
                    assert not got[b - b0].any() and gm[b - b0] == bd.TOO_LONG, (rows.form, b, fill)
                    seen += 1
            mine = [b - b0 for b in range(b0, b0 + n) if b not in longs]
            assert (gm[mine] != bd.TOO_LONG).all() and got[mine].any(1).all()
        assert seen >= len(longs)
    for (g0, m0), (g1, m1) in zip(*res):
        assert np.array_equal(g0, g1) and np.array_equal(m0, m1), rows.form + ": an output word depends on the records of a string without rows"


def long_values(M, strings, flip):
    return {b: (M + 1, 0xffffffff)[(i + flip) % 2] for i, b in enumerate(strings)}


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_strings_without_rows_small_defs(form, flip):
    """regex1 + regex2, M = 19.  G > 1 from Bt strings on, the smallest batch that gets the largest group; the batch's last group holds one string: the first
    and the last place of the first group, the first place of the second, the middle of a group, the last group's only string; a window that begins at string
    3 with a string without rows at its first place, at its first group's last place and alone in its last group.  G = 1 at 300 strings"""
    M = 19
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=0)
    G = cfg.lookup_group(1 << 20)[0]
    Bt = largest_group_from(cfg, G)
    B, n = Bt + 2 * G, Bt                                           # the batch, and a window of it that begins at string 3: both end in a group of one string
    assert G >= 2 and cfg.lookup_group(B) == (G, 1) and cfg.lookup_group(n) == (G, 1) and B % G == 1 and n % G == 1 and 3 + n <= B
    assert cfg.lookup_group(300) == (1, 1)
    chars, lens = ragged_batch(B, M, seed=11)
    rows = rows_of(cfg, form, chars, lens)
    strings = sorted({0, G - 1, G, 3 * G + 1, B - 1, 3, 3 + G - 1, 3 + n - 1})
    no_rows(rows, long_values(M, strings, flip), [(0, None), (3, n)])
    chars, lens = ragged_batch(300, M, seed=12)
    rows = rows_of(cfg, form, chars, lens)
    no_rows(rows, long_values(M, [0, 150, 299, 7], flip), [(0, None), (7, 100)])


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_strings_without_rows_two_big_defs(form, flip):
    """big + big, M = 19: one string per workgroup, four passes — every pass skips the string, the last store writes 0xffffffff"""
    M = bd.M_SMALL
    cfg = bd.configure("big-big", M, 0)
    chars, lens = bd.batch(M)
    assert cfg.lookup_group(len(lens)) == (1, 4)
    rows = rows_of(cfg, form, chars, lens)
    no_rows(rows, long_values(M, [0, bd.LONG, len(lens) - 1], flip), [(0, None), (bd.LONG, 2)])


@pytest.mark.parametrize("form", ["pm", "pm-in"])
def test_strings_without_rows_beside_the_block_border(form):
    """65536 + 300 strings x 19 rows of sweep_def(40), the shape of test_lookup_gpu.test_windows: strings without rows on both sides of the position-major block
    border and at the first place of both windows, in groups of G > 1 and of one"""
    chars, lens = fc.tall_batch()
    B, M = len(lens), 19
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text([fc.sweep_def(fc.BIG_SWEEP_L)]), device=0)
    G = cfg.lookup_group(B)[0]
    n = largest_group_from(cfg, G) + G + 4
    assert G >= 4 and cfg.lookup_group(n)[0] == G and n % G and n + 3 < 65536 and cfg.lookup_group(24)[0] == 1
    rows = rows_of(cfg, form, chars, lens)
    strings = [65528, 65535, 65536, 65551, 3, 3 + G - 1, 3 + n - 1]
    no_rows(rows, long_values(M, strings, 0), [(65528, 24), (3, n)])


# ---- permute: two multi-chunk fill lists per string ---------------------------------------------------------------------------------------------
def device_counts_for_permute(cfg, M):
    """honest device counts of the batch and those of one tamper round's strings"""
    chars, lens = bd.batch(M)
    rows = rows_of(cfg, "pm-in", chars, lens)
    honest = device_counts(rows)[0]
    rnd = bd.tamper_rounds(M, cfg.num_defs - 1)[0]
    for b, (kind, row, d) in rnd.items():
        rows.xor_rec(b, row, d, bd.BITS[kind])
    tampered = device_counts(rows)[0][sorted(rnd)]
    assert not np.array_equal(tampered, honest[sorted(rnd)])
    return honest, tampered


@pytest.mark.parametrize("n_rows", [65537, 65538, 65 * 1024, 65 * 1024 + 1])
def test_permute_two_big_runs(n_rows):
    M = bd.M_SMALL
    cfg = bd.configure("big-big", M, 0)
    p = bd.properties(cfg, 4)
    T, W = t_max(cfg), cfg.lookup_words()
    assert T == p["T"] and n_rows >= T and len(p["big"]) == 2 and p["big"][1][1].start % 4 != 0
    honest, tampered = device_counts_for_permute(cfg, M)
    names, hand, want_over = bd.hand_made(cfg, n_rows)
    counts = np.concatenate([honest, tampered, hand])
    B = len(counts)
    assert cfg.lookup_permute_plan(B, n_rows)["groups"] == 1 and cfg.lookup_permute_workspace_bytes(B, n_rows) == B * W * 4
    got = permute_same_as_host(cfg, counts, n_rows, sample=range(B))                   # indices only, the numpy construction on every string
    over = np.concatenate([np.zeros(B - 4, np.uint32), want_over])
    assert np.array_equal(got["overflow"], over), names
    col = int(np.log2(want_over.max()))
    assert (got["a_idx"][col, B - 1, :n_rows] == NO_ROW).all() and (got["s_idx"][col, B - 1, :n_rows] == NO_ROW).all()
    # cells: the hand-made strings and two honest ones; one table run for the call, then a run per string with distinct challenges
    some = np.concatenate([hand, honest[[4, 7]]])
    one, per_string = host_table(cfg, 0), host_table(cfg, len(some))
    assert not np.array_equal(per_string[0], per_string[1])
    shared = permute_same_as_host(cfg, some, n_rows, one)
    assert not shared["a_cells"][col, 3, :n_rows].any() and not shared["s_cells"][col, 3, :n_rows].any()
    ok = [(c, b) for c in range(6) for b in range(len(some)) if not (c == col and b == 3)]
    for c, b in ok:
        assert np.array_equal(shared["a_idx"][c, b, :n_rows], got["a_idx"][c, B - 4 + b if b < 4 else (4, 7)[b - 4], :n_rows])
    both = permute_same_as_host(cfg, some, n_rows, per_string)
    for c, b in ok[::5]:                                            # the run of the string, not another's
        assert np.array_equal(both["s_cells"][c, b, :n_rows], per_string[b][both["s_idx"][c, b, :n_rows]])
    assert np.array_equal(both["s_idx"], shared["s_idx"])
    if n_rows == 65537:
        # a workspace one byte short, a misaligned one, none: refused, nothing written
        d_counts = torch.from_numpy(counts.view(np.int32)).to(DEV)
        out = Out(cfg, B, n_rows, 0, True, False)
        need = cfg.lookup_permute_workspace_bytes(B, n_rows)
        ws = torch.empty(need + 256, dtype=torch.int8, device=DEV)
        t = out.tensors()
        for bad in (ws[:need - 1], ws[1:need + 1], None):
            rc = hra.lib.hrx_lookup_permute_device(cfg._ctx, d_counts.data_ptr(), B, n_rows, 0, t["a_idx"].data_ptr(), t["s_idx"].data_ptr(), None, 0, None, None,
                                                   t["overflow"].data_ptr(), bad.data_ptr() if bad is not None else None, bad.numel() if bad is not None else 0, None)
            assert rc == hra.HRX_ERR_ARG
        torch.cuda.synchronize()
        assert out.untouched()


# ---- the chain on the device --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["big-big", "big-small-big"])
def test_chain_over_big_runs(oracle, name):
    """counts, compress inputs and table, permute, two invert calls, product — device buffers from stage to stage, as
    test_product_gpu.test_other_def_sets_through_the_device_chain does it.  String 4 has a state of the last def changed, string 6 an end flag of def 0 set,
    string 5 has no rows"""
    M = bd.M_SMALL
    cfg = bd.configure(name, M, 0)
    ref = bd.lookup_ref(oracle, name)
    D, W, ncols = cfg.num_defs, cfg.lookup_words(), 3 * cfg.num_defs
    n_rows = t_max(cfg) + 1
    chars, lens = bd.batch(M)
    B = len(lens)
    rows = rows_of(cfg, "pm-in", chars, lens)
    rows.xor_rec(4, M // 2, D - 1, bd.BITS["state"])
    rows.xor_rec(6, 0, 0, bd.BITS["ee"])
    ch = challenges(3, 23, False)
    theta, beta, gamma = (on_device(c) for c in ch)
    call = dict(layout=rows.layout, planes=rows.planes, **rows.kw)
    raw_c, d_counts = lk_guarded(B * W)
    raw_m, d_misses = lk_guarded(B)
    counts, misses = cfg.lookup_counts(rows.src, rows.d_lens, rows.rec, out=d_counts.view(B, W), misses=d_misses, **call)
    in_cells, raw_i = fc.guarded_cells(torch, DEV, ncols, B, M)
    inputs = cfg.lookup_compress_inputs(rows.src, rows.d_lens, rows.rec, theta, out=in_cells, **call)
    cells, raw = fc.guarded_cells(torch, DEV, 1, 1, W)
    table = cfg.lookup_compress_table(theta, out=cells.view(1, W, 4))[0]
    p_out = Out(cfg, B, n_rows, 0, True, False)
    perm = cfg.lookup_permute(counts, n_rows, out={k: (t if k == "overflow" else t.view(ncols, B, p_out.p)) for k, t in p_out.tensors().items()})
    torch.cuda.synchronize()
    assert lk_intact(raw_c, B * W) and lk_intact(raw_m, B), "a guard of the counts was written"
    fc.guards_intact(raw_i, in_cells, "inputs")
    fc.guards_intact(raw, cells, "table")
    p_out.numpy()                                                   # (the guards and the pitch tails of the index columns)
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    h_table = u64(table)
    ib, ig = device_invert(cfg, h_table, ch[1]), device_invert(cfg, h_table, ch[2])          # (between guards)
    out = Z(ncols, B, n_rows, 0)
    cfg.lookup_product(rows.d_lens, inputs, perm["a_idx"], perm["s_idx"], n_rows, table, on_device(ib), on_device(ig), beta, gamma, out=out.tensors())
    torch.cuda.synchronize()
    got = out.numpy()
    # every stage against its host twin on the same bytes
    rec, msk = rows.host_rows()
    h_counts, h_misses = cfg.lookup_counts_host(chars, lens, rec)
    assert np.array_equal(u32(counts), h_counts) and np.array_equal(u32(misses), h_misses)
    assert np.array_equal(u64(inputs), cfg.lookup_compress_inputs_host(chars, lens, rec, ch[0]))
    assert np.array_equal(h_table, cfg.lookup_compress_table_host(ch[0])[0])
    h_perm = cfg.lookup_permute_host(h_counts, n_rows, out=("idx",))
    a_idx, s_idx = u32(perm["a_idx"]), u32(perm["s_idx"])
    assert np.array_equal(a_idx[:, :, :n_rows], h_perm["a_idx"][:, :, :n_rows]) and np.array_equal(s_idx[:, :, :n_rows], h_perm["s_idx"][:, :, :n_rows])
    assert not u32(perm["overflow"]).any()
    assert np.array_equal(ib, cfg.lookup_invert_table_host(h_table, ch[1])) and np.array_equal(ig, cfg.lookup_invert_table_host(h_table, ch[2]))
    check_inverse_samples(cfg, h_table, ch[1], ib)
    check_inverse_samples(cfg, h_table, ch[2], ig)
    want = cfg.lookup_product_host(lens, u64(inputs), a_idx, s_idx, n_rows, h_table, ib, ig, ch[1], ch[2])
    assert np.array_equal(got["z"][:, :, :n_rows + 1], want["z"][:, :, :n_rows + 1]) and np.array_equal(got["open"], want["open"])
    # the closing property on the honest strings and on the string without rows (zero bins, misses 0xffffffff, zero input cells: every A is the table's first cell)
    one = np.array(cell_limbs(1, False), np.uint64)
    honest = [0, 1, 2, 3, 7]
    assert not h_misses[honest].any() and not got["open"][honest].any() and (got["z"][:, honest, n_rows] == one).all()
    assert h_misses[bd.LONG] == bd.TOO_LONG and not h_counts[bd.LONG].any() and not u64(inputs)[:, bd.LONG].any()
    assert got["open"][bd.LONG] == 0 and (got["z"][:, bd.LONG, n_rows] == one).all()
    # a tampered string opens exactly the lookups that missed
    for b in (4, 6):
        miss = ref.count_records(chars[b], int(lens[b]), M, rec[b])[1]
        bits = sum(1 << (3 * d + k) for d in range(D) for k in range(3) if miss[d, k])
        assert bits and got["open"][b] == bits, (b, miss)
    assert got["open"][4] >> 3 * (D - 1) & 1 and got["open"][6] & 4
    if name == "big-big":                                           # one string in Python integers
        z, opened, ints = pr.product(lookups_of(cfg), lens, M, u64(inputs), a_idx, s_idx, n_rows, h_table, ch[1], ch[2], False, strings=[4])
        assert np.array_equal(got["z"][:, 4, :n_rows + 1], z[:, 4]) and got["open"][4] == opened[4]
