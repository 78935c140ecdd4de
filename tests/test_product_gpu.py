"""LOOKUP PRODUCT on the device (hrx_lookup_invert_table_device / hrx_lookup_product_device, csrc/hrx_kernel_product.hip).  The yardstick is the host twin
(hrx_lookup_invert_table_host / hrx_lookup_product_host over the same cells and index columns copied to the host), limb for limb and word for word; the
host twin itself is held against Python integers in test_product_cpu.py.  Neither is the kernel under test.

  regex1               M = 64, 1, 3 and 5 strings; n_rows around every border of the product kernel's tile (the plan call's tile_rows, in entries of the Z column
                       and in rows), raised to the largest table; z_pitch 0 and 8192; both limb forms; challenges and tables per string and per call
  defs                 regex2 + regex3, five and eight defs, the whole chain on the device and the closing property on its honest strings
  a long table         the synthetic 256-state DFA, 65537 transition rows: the invert kernel walks 65 tiles of one run, the product beyond every tile border
  what goes wrong      a tampered record, permute's overflow pattern, an index of another lookup's range and a zero denominator beside sound lookups
  contract             capture and replay with the calls the first of a fresh context, a side stream, two contexts in turn, refused calls, a host-only context

Every Z column lies between two poisoned 4-KiB guards and the entries above n_rows stay poisoned.  No test provokes a fault: every index that is no word of
its lookup is one the rule answers with a zero term, on the host twin first."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import halo2_regex_amd as hra
import product_ref as pr
from halo2_regex_amd import synth
from compress_ref import R, cell_limbs
from test_compress_gpu import on_device
from test_lookup_gpu import batch
from test_match_cpu import CFG_H4, CFG_23
from test_permute_cpu import lookups_of, t_max
from test_permute_gpu import guarded, intact
from test_product_cpu import Chain, challenges, small_batch
from test_verify_gpu import Rows, defs_of_files, CFG_1

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
NO_ROW = 0xffffffff


def d32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def device_invert(cfg, table, shift, canonical=False, stream=None):
    """the device's inverse table of host arrays, as uint64, between guards"""
    raw, flat = guarded(table.size, torch.int64)
    out = cfg.lookup_invert_table(on_device(table), on_device(shift), out=flat.view(table.shape), canonical=canonical, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert out.data_ptr() == flat.data_ptr() and intact(raw, flat.numel(), torch.int64), "a guard was written"
    return flat.cpu().numpy().view(np.uint64).reshape(table.shape)


class Z:
    """the guarded outputs of one product call"""

    def __init__(self, ncols, b_count, n_rows, z_pitch):
        self.p, self.n_rows, self.shape = z_pitch if z_pitch else (n_rows + 4) & ~3, n_rows, None
        self.shape = (ncols, b_count, self.p, 4)
        self.z, self.open = guarded(int(np.prod(self.shape)), torch.int64), guarded(b_count, torch.int32)

    def tensors(self):
        return {"z": self.z[1], "open": self.open[1]}

    def poison(self):
        self.z[0].fill_(POISON64)
        self.open[0].fill_(POISON32)

    def untouched(self):
        return bool((self.z[0] == POISON64).all()) and bool((self.open[0] == POISON32).all())

    def numpy(self):
        assert intact(self.z[0], self.z[1].numel(), torch.int64) and intact(self.open[0], self.open[1].numel(), torch.int32), "a guard was written"
        z = self.z[1].cpu().numpy().view(np.uint64).reshape(self.shape)
        assert (z[:, :, self.n_rows + 1:] == POISON64).all(), "an entry above n_rows was written"
        return {"z": z, "open": self.open[1].cpu().numpy().view(np.uint32)}


def same_as_host(cfg, lens, inputs, a_idx, s_idx, n_rows, table, beta, gamma, canonical=False, z_pitch=0, b_begin=0):
    """host arrays in; the device's inverse tables and Z against the host twin's, every limb; returns the device outputs"""
    ib, ig = (cfg.lookup_invert_table_host(table, c, canonical=canonical) for c in (beta, gamma))
    gb, gg = (device_invert(cfg, table, c, canonical) for c in (beta, gamma))
    assert np.array_equal(gb, ib) and np.array_equal(gg, ig), "the inverse tables differ from the host twin"
    want = cfg.lookup_product_host(lens, inputs, a_idx, s_idx, n_rows, table, ib, ig, beta, gamma, b_begin=b_begin, z_pitch=z_pitch, canonical=canonical)
    out = Z(inputs.shape[0], inputs.shape[1], n_rows, z_pitch)
    res = cfg.lookup_product(d32(lens), on_device(inputs), d32(a_idx), d32(s_idx), n_rows, on_device(table), on_device(gb), on_device(gg), on_device(beta),
                             on_device(gamma), b_begin=b_begin, z_pitch=z_pitch, canonical=canonical, out=out.tensors())
    torch.cuda.synchronize()
    assert set(res) == {"z", "open"}
    got = out.numpy()
    bad = np.argwhere(got["z"][:, :, :n_rows + 1] != want["z"][:, :, :n_rows + 1])
    assert not len(bad), "z differs from the host twin at %s: n_rows %d, %d strings" % (bad[0], n_rows, inputs.shape[1])
    assert np.array_equal(got["open"], want["open"])
    return got


def host_chain(cfg, B, M, n_rows, canonical=False, per_string=False, seed=1):
    chars, lens = batch(B, M, seed=seed)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    return Chain(cfg, chars, lens, rec, n_rows, canonical, per_string, seed)


def chain_same_as_host(ch, z_pitch=0, **kw):
    return same_as_host(ch.cfg, ch.lens, ch.inputs, kw.get("a_idx", ch.a_idx), kw.get("s_idx", ch.s_idx), ch.n_rows, ch.table, kw.get("beta", ch.beta), ch.gamma,
                        ch.canonical, z_pitch)


# ---- regex1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 5])
def test_regex1_rows_around_every_tile_border(B):
    M = 64
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)
    T = t_max(cfg)
    plan = cfg.lookup_product_plan(B, T)
    tile = plan["tile_rows"]
    assert T == 2843 and tile % plan["rows_per_lane"] == 0
    # tile j - 1, tile j, tile j + 1 for j = 1, 2, raised to the largest table; and the borders that lie above it: a tile is cut in ENTRIES of the Z column
    # (n_rows + 1 of them), so both k tile and k tile - 1 rows are borders
    edges = sorted({max(T, j * tile + s) for j in (1, 2) for s in (-1, 0, 1)} | {T + 1} | {k * tile + s for k in range(T // tile + 1, 4097 // tile + 1) for s in (-2, -1, 0, 1)})
    assert edges[0] == T and edges[-1] == 4097
    for n_rows in edges:
        ch = host_chain(cfg, B, M, n_rows, seed=B)
        got = chain_same_as_host(ch)
        honest = ch.honest()
        assert not got["open"][honest].any()
    ch = host_chain(cfg, B, M, 4090, seed=B)
    got = chain_same_as_host(ch, z_pitch=8192)
    assert got["z"].shape == (3, B, 8192, 4)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("per_string", [False, True])
def test_limb_forms_and_strides(per_string, canonical):
    M = 64
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_23), device=0)
    chars, lens = small_batch(M)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    lens = lens.copy()
    lens[-1] = M + 1                                  # no rows
    ch = Chain(cfg, chars, lens, rec, max(t_max(cfg), M) + 3, canonical, per_string, seed=9)
    got = chain_same_as_host(ch)
    one = np.array(cell_limbs(1, canonical), np.uint64)
    honest = ch.honest()
    assert {0, M, M + 1} <= set(int(lens[b]) for b in honest)
    assert not got["open"][honest].any() and (got["z"][:, honest, ch.n_rows] == one).all()
    # a window of the batch: b_begin
    sub = slice(2, 7)
    w = same_as_host(cfg, lens, np.ascontiguousarray(ch.inputs[:, sub]), np.ascontiguousarray(ch.a_idx[:, sub]), np.ascontiguousarray(ch.s_idx[:, sub]), ch.n_rows,
                     ch.table[sub] if per_string else ch.table, ch.beta[sub] if per_string else ch.beta, ch.gamma[sub] if per_string else ch.gamma, canonical,
                     b_begin=2)
    assert np.array_equal(w["z"], got["z"][:, sub]) and np.array_equal(w["open"], got["open"][sub])


# ---- other def sets: the whole chain on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,names", [("regex23", CFG_23), ("five", CFG_H4 + CFG_23[:1]), ("eight", CFG_H4 * 2)])
def test_other_def_sets_through_the_device_chain(name, names):
    M, B = 64, 4
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(names), device=0)
    n_rows = max(t_max(cfg), M) + 1
    chars, lens = batch(B, M, seed=7)
    rows = Rows(cfg, "pm-in", chars, lens)
    ch = challenges(3, 21, False)
    theta, beta, gamma = (on_device(c) for c in ch)
    counts, misses = cfg.lookup_counts(rows.src, rows.d_lens, rows.rec, layout=rows.layout, planes=rows.planes, **rows.kw)
    inputs = cfg.lookup_compress_inputs(rows.src, rows.d_lens, rows.rec, theta, layout=rows.layout, planes=rows.planes, **rows.kw)
    table = cfg.lookup_compress_table(theta)[0]
    perm = cfg.lookup_permute(counts, n_rows, out=("idx",))
    ib, ig = cfg.lookup_invert_table(table, beta), cfg.lookup_invert_table(table, gamma)
    out = Z(3 * cfg.num_defs, B, n_rows, 0)
    cfg.lookup_product(rows.d_lens, inputs, perm["a_idx"], perm["s_idx"], n_rows, table, ib, ig, beta, gamma, out=out.tensors())
    torch.cuda.synchronize()
    got = out.numpy()
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    want = cfg.lookup_product_host(lens, u64(inputs), u32(perm["a_idx"]), u32(perm["s_idx"]), n_rows, u64(table), u64(ib), u64(ig), ch[1], ch[2])
    assert np.array_equal(got["z"][:, :, :n_rows + 1], want["z"][:, :, :n_rows + 1]) and np.array_equal(got["open"], want["open"])
    assert np.array_equal(u64(ib), cfg.lookup_invert_table_host(u64(table), ch[1]))
    honest = [b for b in range(B) if u32(misses)[b] == 0 and u32(perm["overflow"])[b] == 0]
    assert len(honest) >= 1 and not got["open"][honest].any(), "the closing property through the device chain"
    one = np.array(cell_limbs(1, False), np.uint64)
    assert (got["z"][:, honest, n_rows] == one).all()


# ---- a table of many tiles ----------------------------------------------------------------------------------------------------------------------
def test_the_synthetic_256_state_dfa():
    """65537 transition rows, one string: the invert kernel walks 65 tiles of one run in both passes, the product walks beyond every tile border"""
    a_txt, sub_txt = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=200)
    M = 4096
    cfg = hra.RegexVerifyConfig.configure(M, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub_txt)])], device=0)
    T = t_max(cfg)
    tile = cfg.lookup_product_plan(1, T)["tile_rows"]
    assert T == 65537 and T > 64 * tile
    chars = np.full((1, M), ord("x"), np.uint8)
    lens = np.array([M - 3], np.uint32)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    ch = Chain(cfg, chars, lens, rec, T + 63, seed=4)
    got = chain_same_as_host(ch)
    assert ch.honest() == [0] and got["open"][0] == 0


# ---- what goes wrong ends in `open`, beside sound lookups ---------------------------------------------------------------------------------------
def test_tampered_overflowed_foreign_and_zero_denominator_in_one_window():
    M = 64
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_23), device=0)
    chars, lens = small_batch(M)
    rec, msk, st = cfg.witness_batch_host(chars, lens)
    n_rows = t_max(cfg) + 1
    clean = Chain(cfg, chars, lens, rec, n_rows)
    b0 = next(b for b in clean.honest() if int(lens[b]) == M - 1)
    b1, b2 = [b for b in clean.honest() if b != b0][:2]
    rec = rec.copy()
    rec[b0, 3, 1] = (rec[b0, 3, 1] & ~np.uint32(0xffff)) | np.uint32(0xfff0)          # a state outside every table: def 1's transition lookup of string b0
    ch = Chain(cfg, chars, lens, rec, n_rows)
    looks = lookups_of(cfg)
    a_idx, s_idx = ch.a_idx.copy(), ch.s_idx.copy()
    a_idx[0, b1, :n_rows] = s_idx[0, b1, :n_rows] = NO_ROW                           # permute's overflow pattern
    s_idx[1, b2, 5] = looks[4][1].start                                              # another lookup's range
    a_idx[2, b2, n_rows - 1] = looks[2][1].stop                                      # one behind its own
    got = chain_same_as_host(ch, a_idx=a_idx, s_idx=s_idx)                           # (the host twin ran these indices first)
    zero = np.zeros(4, np.uint64)
    assert got["open"][b0] & 8 and got["open"][b1] == 1 and got["open"][b2] == 6
    assert (got["z"][0, b1, 1:n_rows + 1] == zero).all() and (got["z"][1, b2, 6:n_rows + 1] == zero).all() and got["z"][1, b2, 5].any()
    assert got["z"][2, b2, n_rows - 1].any() and not got["z"][2, b2, n_rows].any()
    others = [b for b in ch.honest() if b not in (b0, b1, b2)]
    assert len(others) >= 1 and not got["open"][others].any()
    # a zero denominator: beta = -S'[j] of lookup 0 of string b1
    S = pr.values_of(ch.table, False)
    beta = np.array(cell_limbs((-S[ch.a_idx[0, b1, 7]]) % R, False), np.uint64)
    got = chain_same_as_host(ch, beta=beta)
    first = int(np.nonzero(ch.a_idx[0, b1, :n_rows] == ch.a_idx[0, b1, 7])[0][0])
    assert got["z"][0, b1, first].any() and (got["z"][0, b1, first + 1:n_rows + 1] == zero).all() and got["open"][b1] & 1


# ---- the invert call alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
def test_invert_against_python_integers_on_samples(canonical):
    cfg = hra.RegexVerifyConfig.configure(64, defs_of_files(CFG_1), device=0)
    W, bins = cfg.lookup_words(), max(sl.stop for _, sl in lookups_of(cfg))
    thetas = challenges(3, 5, canonical)
    table = cfg.lookup_compress_table_host(thetas, canonical=canonical)
    S0 = pr.values_of(table[0, :8], canonical)
    shifts = np.array([cell_limbs(c, canonical) for c in (0, (-S0[5]) % R, R - 1)], np.uint64)       # run 1: word 5 of run 0's value need not be zero there
    shifts[1] = cell_limbs((-pr.value_of(table[1, 5], canonical)) % R, canonical)
    inv = device_invert(cfg, table, shifts, canonical)
    assert np.array_equal(inv, cfg.lookup_invert_table_host(table, shifts, canonical=canonical))
    rng = np.random.default_rng(3)
    for t in range(3):
        c = pr.challenge_value(shifts[t], canonical)
        for w in sorted(set(rng.integers(0, bins, 40).tolist()) | {0, 5, 1023, 1024, 2047, 2048, bins - 1}):
            s = (pr.value_of(table[t, w], canonical) + c) % R
            assert pr.value_of(inv[t, w], canonical) == (pow(s, -1, R) if s else 0), (t, w)
        assert not inv[t, bins:].any()
    assert not inv[1, 5].any()
    one = device_invert(cfg, table[2], shifts[2], canonical)                                             # one run, one shift for the call
    assert np.array_equal(one, inv[2])


# ---- the contract -------------------------------------------------------------------------------------------------------------------------------
def test_capture_replay_as_the_first_calls_of_a_fresh_context_and_a_side_stream():
    M = 64
    src = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=hra.HRX_DEVICE_NONE)
    n_rows = t_max(src) + 1
    ch = host_chain(src, 3, M, n_rows, seed=2)
    want = ch.product()
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)           # no call of any kind on it before the capture
    d = dict(lens=d32(ch.lens), inputs=on_device(ch.inputs), a=d32(ch.a_idx), s=d32(ch.s_idx), table=on_device(ch.table), beta=on_device(ch.beta), gamma=on_device(ch.gamma))
    raw_b, ib = guarded(ch.table.size, torch.int64)
    raw_g, ig = guarded(ch.table.size, torch.int64)
    ib, ig = ib.view(ch.table.shape), ig.view(ch.table.shape)
    out = Z(3, 3, n_rows, 0)
    side = torch.cuda.Stream(DEV)

    def run(stream):
        cfg.lookup_invert_table(d["table"], d["beta"], out=ib, stream=stream)
        cfg.lookup_invert_table(d["table"], d["gamma"], out=ig, stream=stream)
        cfg.lookup_product(d["lens"], d["inputs"], d["a"], d["s"], n_rows, d["table"], ib, ig, d["beta"], d["gamma"], out=out.tensors(), stream=stream)

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        run(side)
    torch.cuda.synchronize()
    assert out.untouched() and bool((raw_b == POISON64).all())                          # captured, not run
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        got = out.numpy()
        assert np.array_equal(got["z"][:, :, :n_rows + 1], want["z"][:, :, :n_rows + 1]) and np.array_equal(got["open"], want["open"])
        assert np.array_equal(ib.cpu().numpy().view(np.uint64), ch.inv_beta) and intact(raw_g, ig.numel(), torch.int64)
        out.poison()
        raw_b.fill_(POISON64)
    run(side)                                                                           # eager, on the side stream
    side.synchronize()
    assert np.array_equal(out.numpy()["z"][:, :, :n_rows + 1], want["z"][:, :, :n_rows + 1])


def test_the_chain_on_two_contexts_used_alternately():
    M, B = 64, 3
    cfgs = [hra.RegexVerifyConfig.configure(M, defs_of_files(names), device=0) for names in (CFG_1, CFG_23)]
    chars, lens = batch(B, M, seed=5)
    d_chars, d_lens = torch.from_numpy(chars).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV)
    ch = challenges(3, 13, False)
    theta, beta, gamma = (on_device(c) for c in ch)
    st = [dict() for _ in cfgs]
    for step in range(6):
        for i, cfg in enumerate(cfgs):
            s, n_rows = st[i], t_max(cfg) + 1
            if step == 0:
                s["rec"] = cfg.witness_batch(d_chars, d_lens)[0]
            elif step == 1:
                s["counts"], s["misses"] = cfg.lookup_counts(d_chars, d_lens, s["rec"])
            elif step == 2:
                s["table"], s["inputs"] = cfg.lookup_compress_table(theta)[0], cfg.lookup_compress_inputs(d_chars, d_lens, s["rec"], theta)
            elif step == 3:
                s["perm"] = cfg.lookup_permute(s["counts"], n_rows, out=("idx",))
            elif step == 4:
                s["ib"], s["ig"] = cfg.lookup_invert_table(s["table"], beta), cfg.lookup_invert_table(s["table"], gamma)
            else:
                s["res"] = cfg.lookup_product(d_lens, s["inputs"], s["perm"]["a_idx"], s["perm"]["s_idx"], n_rows, s["table"], s["ib"], s["ig"], beta, gamma)
    torch.cuda.synchronize()
    for i, cfg in enumerate(cfgs):
        n_rows = t_max(cfg) + 1
        rec = st[i]["rec"].cpu().numpy().view(np.uint32)
        host = Chain(cfg, chars, lens, rec, n_rows)
        host.theta, host.beta, host.gamma = ch
        host.table = cfg.lookup_compress_table_host(ch[0])[0]
        host.inputs = cfg.lookup_compress_inputs_host(chars, lens, rec, ch[0])
        host.inv_beta, host.inv_gamma = cfg.lookup_invert_table_host(host.table, ch[1]), cfg.lookup_invert_table_host(host.table, ch[2])
        want = host.product()
        z = st[i]["res"]["z"].cpu().numpy().view(np.uint64)
        assert np.array_equal(st[i]["ib"].cpu().numpy().view(np.uint64), host.inv_beta)
        assert np.array_equal(z[:, :, :n_rows + 1], want["z"][:, :, :n_rows + 1]), i
        assert np.array_equal(st[i]["res"]["open"].cpu().numpy().view(np.uint32), want["open"])
        assert not want["open"][host.honest()].any()


def test_refused_calls_write_nothing_and_a_host_only_context():
    M = 19
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_23), device=0)
    B, W, T, ncols = 2, cfg.lookup_words(), t_max(cfg), 3 * cfg.num_defs
    n_rows = max(T, M) + 2
    ip, zp = (n_rows + 3) & ~3, (n_rows + 4) & ~3
    lens = torch.tensor([3, 19], dtype=torch.int32, device=DEV)
    inputs = torch.zeros((ncols, B, M, 4), dtype=torch.int64, device=DEV)
    idx = torch.zeros((ncols, B, ip), dtype=torch.int32, device=DEV)
    tabs = torch.zeros((3, W, 4), dtype=torch.int64, device=DEV)
    bg = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    out = Z(ncols, B, n_rows, zp)
    t = out.tensors()
    good = dict(lens=lens.data_ptr(), M=M, b_begin=0, b_count=B, in_cells=inputs.data_ptr(), a_idx=idx.data_ptr(), s_idx=idx.data_ptr(), n_rows=n_rows, idx_pitch=ip,
                table=tabs[0].data_ptr(), ib=tabs[1].data_ptr(), ig=tabs[2].data_ptr(), tstride=0, beta=bg[0].data_ptr(), gamma=bg[1].data_ptr(), cstride=0,
                z=t["z"].data_ptr(), z_pitch=zp, open=t["open"].data_ptr(), flags=0)
    order = list(good)

    def call(ctx=cfg._ctx, **kw):
        a = dict(good, **kw)
        return hra.lib.hrx_lookup_product_device(ctx, *[a[k] for k in order], None)

    bad = [dict(n_rows=T - 1), dict(n_rows=(1 << 24) + 1, idx_pitch=0, z_pitch=0), dict(idx_pitch=ip - 4), dict(idx_pitch=ip + 2), dict(z_pitch=n_rows), dict(z_pitch=zp + 2),
           dict(tstride=4), dict(cstride=8), dict(flags=2), dict(lens=None), dict(in_cells=None), dict(s_idx=None), dict(ig=None), dict(gamma=None), dict(z=None),
           dict(in_cells=good["in_cells"] + 8), dict(a_idx=good["a_idx"] + 4), dict(ib=good["ib"] + 8), dict(z=good["z"] + 8), dict(open=good["open"] + 2)]
    for kw in bad:
        assert call(**kw) == hra.HRX_ERR_ARG, kw
    assert call(ctx=None) == hra.HRX_ERR_ARG
    host_only = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_23), device=hra.HRX_DEVICE_NONE)
    assert call(ctx=host_only._ctx) == hra.HRX_ERR_HIP
    raw, inv = guarded(W * 4, torch.int64)
    gi = hra.lib.hrx_lookup_invert_table_device
    for args in [(None, 1, bg.data_ptr(), 0, inv.data_ptr(), 0, None, 0), (tabs.data_ptr(), 1, None, 0, inv.data_ptr(), 0, None, 0), (tabs.data_ptr(), 1, bg.data_ptr(), 0, None, 0, None, 0),
                 (tabs.data_ptr() + 8, 1, bg.data_ptr(), 0, inv.data_ptr(), 0, None, 0), (tabs.data_ptr(), 1, bg.data_ptr(), 8, inv.data_ptr(), 0, None, 0),
                 (tabs.data_ptr(), 1, bg.data_ptr(), 0, inv.data_ptr(), 2, None, 0), (tabs.data_ptr(), 1, bg.data_ptr(), 0, inv.data_ptr(), 0, tabs.data_ptr() + 64, 4096)]:
        assert gi(cfg._ctx, *args, None) == hra.HRX_ERR_ARG, args
    assert gi(host_only._ctx, tabs.data_ptr(), 1, bg.data_ptr(), 0, inv.data_ptr(), 0, None, 0, None) == hra.HRX_ERR_HIP
    torch.cuda.synchronize()
    assert out.untouched() and bool((raw == POISON64).all())
    assert call(b_count=0) == hra.HRX_OK and call() == hra.HRX_OK and gi(cfg._ctx, tabs.data_ptr(), 1, bg.data_ptr(), 0, inv.data_ptr(), 0, None, 0, None) == hra.HRX_OK
    torch.cuda.synchronize()
    got = out.numpy()
    assert (got["z"][:, :, :n_rows + 1] != POISON64).all() and not inv.any() and intact(raw, inv.numel(), torch.int64)
